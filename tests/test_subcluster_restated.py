"""CPU: the restatement of BayesHammer's subclustering (tests/subcluster_restated.py) pinned on its own, before anything
is compared with it: the tables against hand values, hand-worked clusters against a plain formula for the BIC, and every
crafted case of tests/subcluster_cases.py against the branch it was built to take."""
import math

import numpy as np
import pytest

from tests import subcluster_cases as Cs
from tests import subcluster_restated as R

KS = [21, 32]


def test_tables_equal_hand_values():
    probs, lprobs, rprobs, lrprobs = R.tables()
    assert len(probs) == 256
    assert R.LP[0] == math.log(0.25) and R.LP[2] == math.log(0.25)
    assert R.LR3[0] == math.log(0.75) - math.log(3)
    assert rprobs[40] == math.pow(10.0, -4.0) and R.LR3[40] == math.log(math.pow(10.0, -40 / 10.0)) - math.log(3)
    assert R.LR3[40] == math.log(1e-4) - math.log(3)
    assert R.LP[3] == math.log(1 - math.pow(10.0, -0.3))
    assert R.LP[63] == math.log(1 - math.pow(10.0, -6.3))


def test_quality_words_round_trip():
    for k in (10, 11, 21, 22, 32):
        q = [(7 * i + 3) % 64 for i in range(k)]
        w = R.pack_quals(q)
        assert len(w) == (6 * k + 63) // 64 and R.quals_of(w, k) == q
    # sum 10 straddles words 0 and 1 (bits 60 .. 65)
    assert R.pack_quals([0] * 10 + [63]) == [0xF << 60, 0x3]


def _logl(kmer, quals, center):
    """the plain formula: left to right from 0.0"""
    r = 0.0
    for a, b, q in zip(kmer, center, quals):
        r += R.LP[q] if a == b else R.LR3[q]
    return r


def _bic(ll_terms, l, k, total):
    loglik = 0.0
    for cnt, ll in ll_terms:
        loglik += cnt * ll
    return loglik - float(3 * l * k + l - 1) * math.log(float(total)) / 2.0


def test_hand_worked_pair():
    """two k-mers one substitution apart, counts 40 and 2, good qualities: one cluster around the first; BIC(1) by the
    plain formula, and BIC(2) < BIC(1) is why l = 1 stands (maxcls = 2 stops the loop at l = 2)"""
    k = 21
    a = R.key_of([i % 4 for i in range(k)])
    b = Cs.sub(a, 5, 1)
    qa, qb = [40] * k, [20] * k
    case = Cs.make_case(k, [(a, 40, np.float32(1e-6), qa), (b, 2, np.float32(0.5), qb)], [[0, 1]])
    r = Cs.restate(case)
    sa, sb = R.bases(a, k), R.bases(b, k)
    bic1 = _bic([(40, _logl(sa, qa, sa)), (2, _logl(sb, qb, sa))], 1, k, 42)
    bic2 = _bic([(40, _logl(sa, qa, sa)), (2, _logl(sb, qb, sb))], 2, k, 42)
    assert bic2 < bic1
    assert r["bic"].view(np.uint64).tolist() == np.array([bic1]).view(np.uint64).tolist()
    ia, ib = case["keys"].index(a), case["keys"].index(b)
    assert r["members"].tolist() == [ia, ib] and r["sizes"].tolist() == [2] and r["per_cluster"].tolist() == [1]
    # center_quality = 1 - 1e-6f > 0.995 and cluster_quality = 1 - 0.5 is not above 0.9: correct_threshold 0.98 decides
    assert r["good"].tolist() == ([1, 0] if ia == 0 else [0, 1])
    assert dict(zip("gsingl tsingl tcsingl gcsingl tcls gcls tkmers tncls newkmers".split(), r["stats"].tolist())) == dict(
        gsingl=0, tsingl=0, tcsingl=0, gcsingl=0, tcls=1, gcls=0, tkmers=2, tncls=1, newkmers=0)
    errs = np.zeros(16, dtype=np.uint64)
    for x, y in zip(sa, sb):
        errs[4 * x + y] += 1
    assert r["errs"].tolist() == errs.tolist()
    assert "maxcls_stop" in r["trace"]


def test_hand_worked_triple():
    """three k-mers: two strong ones four substitutions apart and a weak neighbour of the second: two subclusters, the
    BIC of l = 2 by the plain formula"""
    k = 21
    a = R.key_of([(3 * i) % 4 for i in range(k)])
    b = a
    for p in (2, 7, 11, 16):
        b = Cs.sub(b, p, 2)
    c = Cs.sub(b, 19, 1)
    qa, qb, qc = [45] * k, [45] * k, [10] * k
    case = Cs.make_case(k, [(a, 60, np.float32(1e-7), qa), (b, 50, np.float32(1e-7), qb), (c, 1, np.float32(0.05), qc)],
                        [[0, 1, 2]])
    r = Cs.restate(case)
    sa, sb, sc = (R.bases(x, k) for x in (a, b, c))
    bic2 = _bic([(60, _logl(sa, qa, sa)), (50, _logl(sb, qb, sb)), (1, _logl(sc, qc, sb))], 2, k, 111)
    assert r["bic"].view(np.uint64).tolist() == np.array([bic2]).view(np.uint64).tolist()
    ia, ib, ic = (case["keys"].index(x) for x in (a, b, c))
    assert r["members"].tolist() == [ia, ib, ic] and r["sizes"].tolist() == [1, 2]
    assert "one_member_subcluster" in r["trace"]
    # a: singleton subcluster, 1 > 0.9 and quality good; b: cluster_quality = 1 - 0.05 = 0.95 > 0.9
    assert [int(r["good"][i]) for i in (ia, ib, ic)] == [1, 1, 0]
    st = dict(zip("gsingl tsingl tcsingl gcsingl tcls gcls tkmers tncls newkmers".split(), r["stats"].tolist()))
    assert st == dict(gsingl=0, tsingl=0, tcsingl=1, gcsingl=1, tcls=1, gcls=1, tkmers=3, tncls=1, newkmers=0)


@pytest.mark.parametrize("k", KS)
def test_crafted_cases_take_their_branch(k):
    for name, (case, params, want) in Cs.crafted(k).items():
        r = Cs.restate(case, params)
        assert want <= r["trace"], (name, sorted(r["trace"]))


@pytest.mark.parametrize("k", KS)
def test_new_kmer_appears_and_ends_bad(k):
    case = Cs.chain_case(k)
    assert case["count"].tolist().count(10) == 3 and case["count"].tolist().count(1) == 2
    r = Cs.restate(case)
    n = len(case["keys"])
    assert len(r["new_keys"]) == 1 and int(r["new_keys"][0]) not in case["keys"]
    assert r["members"][0] == n and r["sizes"].tolist() == [6] and len(r["good"]) == n + 1 and r["good"][n] == 0
    assert r["stats"].tolist()[-1] == 1


@pytest.mark.parametrize("k", KS)
def test_searched_cases_exist(k):
    """the cases found by search are registered under their names at both k; that each takes its branch is asserted by
    test_crafted_cases_take_their_branch"""
    names = set(Cs.crafted(k))
    assert {"center_without_members", "one_member_subcluster", "maxcls_stop", "listed_twice", "duplicate_center"} <= names


def test_center_without_members_is_all_a():
    trace = set()
    kmers = [R.ExpandedKMer(R.key_of([1] * 21), 21, 3, [30] * 21), R.ExpandedKMer(R.key_of([2] * 21), 21, 4, [30] * 21)]
    assert R.consensus_with_mask(kmers, [0, 0], 1, 21, trace) == [0] * 21 and trace == {"center_without_members"}
    assert R.consensus_with_mask(kmers[:1], [0], 1, 21, trace) == [1] * 21  # the size of the block decides, not the mask


def test_ties_are_resolved_by_index():
    """equal counts: after the center, the members of every list ascend by index"""
    case = Cs.tie_case(21)
    r = Cs.restate(case)
    assert case["sizes"].tolist() == [6, 6, 6] and "count_tie" in r["trace"]
    p = 0
    for sz in r["sizes"].tolist():
        rest = r["members"][p + 1:p + sz].tolist()
        assert rest == sorted(rest)
        p += sz


@pytest.mark.parametrize("k", KS)
def test_threshold_equality_is_strict_and_float(k):
    case, p = Cs.threshold_case(k)
    r = Cs.restate(case, p)
    f = np.float32
    by_tq = {}
    o = 0
    for size in case["sizes"].tolist():
        if size == 1:
            i = int(case["members"][o])
            by_tq[float(case["tq"][i])] = int(r["good"][i])
        o += size
    down, up = (lambda x: float(np.nextafter(f(x), f(-1)))), (lambda x: float(np.nextafter(f(x), f(2))))
    e = f(2.0 ** -24)
    # against correct_threshold 0.5: 1 - 0.5 is not above it; 0.5 - 2^-24 gives the float 0.5 + 2^-24, which is
    assert by_tq[0.5] == 0 and by_tq[float(f(0.5) - e)] == 1 and by_tq[up(0.5)] == 0
    # the float below 0.5: the double difference 0.5 + 2^-25 is above 0.5, the float one is a tie that rounds to 0.5
    t = f(down(0.5))
    assert 1.0 - float(t) > 0.5 and float(f(1) - t) == 0.5 and by_tq[float(t)] == 0
    assert by_tq[0.0] == 1 and by_tq[1.0] == 0
    # against singleton_threshold 0.75 everything here is good through correct_threshold; gsingl tells
    assert by_tq[0.25] == by_tq[up(0.25)] == by_tq[down(0.25)] == by_tq[float(f(0.25) - e)] == 1
    assert r["stats"][0] == 2 and r["stats"][1] == 10  # gsingl: tq 0 and 0.25 - 2^-24
    t = f(down(0.25))  # 0.25 - 2^-26: in double 0.75 + 2^-26, in float 0.75
    assert 1.0 - float(t) > 0.75 and float(f(1) - t) == 0.75
    assert R.decide_singleton(t, p) == (1, 0) and R.decide_singleton(f(0.25) - e, p) == (1, 1)
    assert R.decide_singleton(f(0.25), p) == (1, 0) and R.decide_singleton(f(up(0.25)), p) == (1, 0)
    # the pairs: the member's total_qual 0.125 puts cluster_quality exactly at 0.875: not above
    assert R.decide_center(f(0.125), [f(0.125)], p)[:2] == (1, 0)
    assert R.decide_center(f(0.125), [f(down(0.125))], p)[:2] == (1, 1)
    assert R.decide_center(f(0.25), [f(down(0.125))], p)[:2] == (1, 0)  # center_quality 0.75 is at its threshold
    assert R.decide_center(f(0.5), [f(down(0.125))], p)[:2] == (0, 0)  # and 0.5 at correct_threshold
    assert r["stats"][5] == 1  # of the twelve pairs only (0.125, below 0.125) is a good cluster


@pytest.mark.parametrize("k", KS)
def test_denormal_total_qual_in_the_product(k):
    case = Cs.denormal_case(k)
    assert (case["tq"][case["tq"] > 0] < np.float32(1.1754944e-38)).sum() == 3  # 1.1754942e-38 is the largest denormal
    r = Cs.restate(case)
    assert r["stats"][5] == 3  # 1 - (a product around 1e-46) is 1.0 in double: all three are good clusters
    g, c, q = R.decide_center(np.float32(1e-4), [np.float32(0.3), np.float32(1e-45), np.float32(0.5)], R.DEFAULTS)
    assert (g, c) == (1, 1) and q == 1 - 0.30000001192092896 * 1.401298464324817e-45 * 0.5


def test_fused_multiply_add_changes_a_bic():
    """what the GPU test's docstring claims: with `loglik += count * logL` contracted into one fused operation the BIC of
    a cluster of the count_ties case has other bits (k = 21 and k = 32), so that case catches a build that contracts"""
    for k in KS:
        case = Cs.tie_case(k)
        a, b = Cs.restate(case), Cs.restate(case, mul_add=R.fused)
        assert (a["bic"].view(np.uint64) != b["bic"].view(np.uint64)).any()
