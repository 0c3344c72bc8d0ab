"""CPU: the Python restatements of the BayesHammer chain against tests/golden/hammer_ref/, the outputs of the
reference's own code (recorded by oracle/record_hammer_ref.py through oracle/hammer_ref_driver.cpp, one thread, K = 21,
tau = 1, one iteration, no singleton filter).  Every restatement is given the REFERENCE's recorded output of the stage
before it and has to reproduce the reference's recorded output of its own stage, so one wrong stage cannot hide the next.

No GPU, no engine, no reference tree: only the last test (the drift guard) runs the reference binary, and skips without it.

Measured on the committed fixtures (profiles/hammer_ref/README.md): total_qual of the restatement and of the reference are
bit-equal for every k-mer of both cases; the worst |reference - exact product| / bound is 0.094.
"""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import expander_restated as E
from tests import hamcluster_restated as H
from tests import hammer_ref_case as C
from tests import hreads_restated as HR
from tests import kmerdata_restated as KR
from tests import readcorrect_restated as R
from tests import readprint_restated as P
from tests import subcluster_restated as S

K = C.K
TRIM = 4  # input_trim_quality of tests/golden/hammer_config.info
OFFSET = 33

_CACHE = {}


def fx(case, stage):
    if (case, stage) not in _CACHE:
        _CACHE[case, stage] = C.load(case, stage)
    return _CACHE[case, stage]


def records(case):
    """[left records, right records] as the reference's parser hands them on"""
    if ("records", case) not in _CACHE:
        left, right, _ = C.case_texts(case)
        _CACHE["records", case] = [C.parsed(left, OFFSET), C.parsed(right, OFFSET)]
    return _CACHE["records", case]


def reads_in_order(case):
    """(seq, qual) of every read in the order every stage of the reference walks them: the left file, then the right"""
    left, right = records(case)
    return [(s, q) for _, s, q in left + right]


def ascending(case):
    """(k-mers ascending by the engine's key, {k-mer: position}, positions of stage1.tsv's rows)"""
    if ("asc", case) not in _CACHE:
        kmers = fx(case, "stage1")["kmers"]
        order = sorted(range(len(kmers)), key=lambda i: KR.kmer_key(kmers[i]))
        asc = [kmers[i] for i in order]
        _CACHE["asc", case] = (asc, {x: i for i, x in enumerate(asc)}, order)
    return _CACHE["asc", case]


def good_of(case, bits):
    """a good-bit string in the order of stage3.tsv -> list over the ascending set"""
    asc, pos, _ = ascending(case)
    kmers = fx(case, "stage3")["kmers"]
    good = [0] * len(asc)
    for km, b in zip(kmers[:len(asc)], bits):
        good[pos[km]] = int(b)
    return good


def sizes_of(case):
    return [len(c) for c in fx(case, "stage2")["clusters"]]


# ---- the conditions the inputs were built to meet, from the reference's output alone --------------------------------------
@pytest.mark.parametrize("case", C.CASES)
def test_inputs_are_the_recorded_ones(case):
    left, right, names = C.case_texts(case)
    prov = fx(case, "stage5")["_provenance"]
    assert prov["input_md5"] == {names[0]: C.md5(left), names[1]: C.md5(right)}
    assert prov["threads"] == dict.fromkeys(prov["threads"], 1) and prov["overrides"]["count_filter_singletons"] == 0
    for stage in ("stage0",) + C.STAGES[1:]:
        assert fx(case, stage)["_provenance"] == prov
    assert len(fx(case, "stage3")["kmers"]) == len(fx(case, "stage1")["kmers"]) + len(fx(case, "stage3")["new_centres"])


@pytest.mark.parametrize("case", C.CASES)
def test_reference_reached_the_closure(case):
    s4 = fx(case, "stage4")
    assert s4["extra_pass_added"] == 0
    assert s4["rounds"][-1]["added"] < 10 and all(r["added"] >= 10 for r in s4["rounds"][:-1])
    assert sum(r["added"] for r in s4["rounds"]) > 0


def test_size_classes_are_present():
    sizes = sizes_of("crafted")
    assert any(s == 1 for s in sizes) and any(1 < s <= 64 for s in sizes) and any(64 < s <= 256 for s in sizes)
    assert max(sizes) < 2500  # no component replay
    assert any(1 < s <= 64 for s in sizes_of("ecoli"))


def test_corrector_takes_every_route():
    s5 = fx("crafted", "stage5")
    names = C.case_texts("crafted")[2]
    base = [n[:-len(".fastq")] for n in names]
    cor, unp, bad = ("%s.00.0_0.cor.fastq" % base[0], "crafted__unpaired.00.0_0.cor.fastq", "%s.00.bad.fastq" % base[0])
    for f in (cor, unp, bad, "%s.00.bad.fastq" % base[1]):
        assert s5["files"][f].count("\n") >= 4, f
    assert any(" BH:changed:" in text for text in s5["files"].values())  # a base was changed
    assert s5["changed_reads"] > 0 and fx("ecoli", "stage5")["changed_reads"] > 0
    assert s5["dataset"] == [["left", cor], ["right", "%s.00.0_0.cor.fastq" % base[1]], ["single", unp]]


# ---- stage 0: trims, valid starts, Read::print ----------------------------------------------------------------------------
def _stage0_rows(case):
    recs = records(case)
    rows = fx(case, "stage0")["reads"]
    assert [r["file"] for r in rows] == [0] * len(recs[0]) + [1] * len(recs[1])
    return list(zip(rows, recs[0] + recs[1]))


@pytest.mark.parametrize("case", C.CASES)
def test_stage0_trims(case):
    seen = set()
    for row, (name, seq, qual) in _stage0_rows(case):
        assert row["name"] == name
        want = (row["ltrim"], row["rtrim"], row["initial_size"], row["size"])
        s, q, ltrim_, rtrim_, initial = R.trim_read(seq, list(qual), TRIM)
        assert (ltrim_, rtrim_, initial, len(s)) == want, name
        s2, q2, lt = KR.trim_ns_and_bad_quality(seq, list(qual), TRIM)
        assert (s2, list(q2)) == (s, list(q)), name
        if len(s):
            assert lt == row["ltrim"], name
        span = (row["ltrim"], row["size"]) if row["size"] else (0, 0)
        assert HR.literal_trim(seq, qual, TRIM) == span, name
        assert HR.closed_trim(seq, qual, TRIM) == span, name
        seen.add("empty" if not row["size"] else "k" if row["size"] == K else "k-1" if row["size"] == K - 1 else
                 "both" if row["ltrim"] and row["rtrim"] < initial else "left" if row["ltrim"] else
                 "right" if row["rtrim"] < initial else "whole")
    assert seen >= ({"empty", "k", "k-1", "both", "left", "right", "whole"} if case == "crafted" else {"right", "whole"})


@pytest.mark.parametrize("case", C.CASES)
def test_stage0_valid_starts_and_probabilities(case):
    gaps = 0
    for row, (name, seq, qual) in _stage0_rows(case):
        s, q, _, _, _ = R.trim_read(seq, list(qual), TRIM)
        q4 = dict(zip(row["starts_q2"], row["probs_q2"]))
        q4 = {st: q4.get(st) for st in row["starts_q4"]}
        q4.update({st: p for st, p in row["probs_q4_where_not_q2"]})
        for threshold, starts, probs in ((2, row["starts_q2"], row["probs_q2"]),
                                         (4, row["starts_q4"], [q4[st] for st in row["starts_q4"]])):
            gen = KR.ValidKMerGenerator(s, q, K, threshold)
            got = []
            while gen.has_more():
                got.append((gen.pos() - 1, gen.correct_probability_))
                gen.next()
            assert [g[0] for g in got] == starts, (name, threshold)
            assert [g[1] for g in got] == probs, (name, threshold)  # the same doubles: the same operations in the same order
        if len(s) >= K:
            assert [x - row["ltrim"] for x in KR.valid_starts(seq, list(qual), K, TRIM)] == row["starts_q2"], name
        assert HR.literal_starts(s, q, K, HR.is_nucl_kmer) == row["starts_q2"], name
        assert HR.closed_starts(s, q, K, HR.is_nucl_kmer) == row["starts_q2"], name
        gaps += len(KR.coalesce(row["starts_q2"], K)) > 1
    assert gaps or case != "crafted"  # a read with an N inside: more than one stretch


@pytest.mark.parametrize("case", C.CASES)
def test_stage0_printed_text(case):
    for side, recs in enumerate(records(case)):
        text = ""
        for name, seq, qual in recs:
            s, q, ltrim_, rtrim_, initial = R.trim_read(seq, list(qual), TRIM)
            text += R.read_print(name, s, q, ltrim_, rtrim_, initial, OFFSET)
        assert text == fx(case, "stage0")["printed"][side]
    if case == "crafted":
        both = "".join(fx(case, "stage0")["printed"])
        # p13/1: 40 bad bases, k good ones, 39 bad ones -- the reference keeps the right end (read.hpp:101)
        assert " ltrim=40\n" in both and re.search(r" ltrim=\d+ rtrim=\d+\n", both) and "\n+p0/1 rtrim=" in both


# ---- stage 1: KMerStat filling ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES)
def test_stage1_statistics(case):
    s1 = fx(case, "stage1")
    data = KR.fill_kmer_data(reads_in_order(case), K, trim_quality=TRIM)
    assert sorted(data) == s1["kmers"]  # the set itself: the count step of the reference found the same k-mers
    worst, equal, saturated = Fraction(0), 0, 0
    for km, count, bits, words in zip(s1["kmers"], s1["count"], s1["total_qual_bits"], s1["qual_words"]):
        st = data[km]
        assert st.count == count, km
        assert ["%016x" % w for w in st.qual.words()] == words, km
        saturated += 63 in st.qual.values()
        ref = Fraction(float(np.array([int(bits, 16)], dtype=np.uint32).view(np.float32)[0]))
        exact, bound = KR.total_qual_bound(st.factors)
        assert abs(ref - exact) <= bound, km
        assert abs(Fraction(float(st.total_qual)) - exact) <= bound, km
        worst = max(worst, abs(ref - exact) / bound)
        equal += Fraction(float(st.total_qual)) == ref
    print("%s: total_qual worst |reference - exact| / bound = %.4f, bit-equal to the restatement: %d of %d, k-mers with a "
          "saturated quality sum: %d" % (case, float(worst), equal, len(s1["kmers"]), saturated))
    assert saturated  # the saturating end of the sum is exercised


# ---- stage 2: tau = 1 Hamming clusters -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES)
def test_stage2_partition(case):
    asc, pos, _ = ascending(case)
    keys = [KR.kmer_key(x) for x in asc]
    assert keys == H.both_strands(keys, K)
    lab = H.cluster(keys, K)
    groups = {}
    for i, l in lab.items():
        groups.setdefault(l, set()).add(asc[i])
    want = {frozenset(c) for c in fx(case, "stage2")["clusters"]}
    assert sum(len(c) for c in want) == len(asc)
    assert {frozenset(g) for g in groups.values()} == want


# ---- stage 3: Bayesian subclustering ---------------------------------------------------------------------------------------
def _stage3_inputs(case):
    """the reference's recorded statistics and clusters as subcluster_restated.process takes them"""
    asc, pos, order = ascending(case)
    s1 = fx(case, "stage1")
    count = [s1["count"][i] for i in order]
    tq = np.array([int(s1["total_qual_bits"][i], 16) for i in order], dtype=np.uint32).view(np.float32)
    words = [[int(w, 16) for w in s1["qual_words"][i]] for i in order]
    clusters = fx(case, "stage2")["clusters"]
    members = [pos[x] for c in clusters for x in c]
    return asc, pos, count, tq, words, members, [len(c) for c in clusters]


@pytest.mark.parametrize("case", C.CASES)
def test_stage3_good_bits_and_new_centres(case):
    asc, pos, count, tq, words, members, sizes = _stage3_inputs(case)
    out = S.process([KR.kmer_key(x) for x in asc], K, count, tq, words, members, sizes)
    s3 = fx(case, "stage3")
    want = good_of(case, s3["good"])
    got = [int(x) for x in out["good"][:len(asc)]]
    wrong = [asc[i] for i in range(len(asc)) if got[i] != want[i]]
    assert wrong == [], "%d k-mers differ, first %s" % (len(wrong), wrong[:5])
    # new centres: the reference numbers them in the order of its cluster file, which follows its hash; compared as a set
    new_good = dict(zip(s3["new_centres"], (int(b) for b in s3["good"][len(asc):])))
    assert len(new_good) == len(s3["new_centres"]) == len(out["new_keys"])
    assert {KR.kmer_key(x): g for x, g in new_good.items()} == \
        dict(zip((int(x) for x in out["new_keys"]), (int(x) for x in out["good"][len(asc):])))
    assert [s3["count"][s3["kmers"].index(x)] for x in asc[:50]] == count[:50]
    if case == "crafted":
        assert {"count_tie", "maxcls_stop", "new_kmer"} <= out["trace"] and len(new_good) == 2 and not set(new_good) & set(asc)


# ---- stage 4: the Expander ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES)
def test_stage4_in_place_rounds_and_snapshot_closure(case):
    asc, pos, _ = ascending(case)
    reads = reads_in_order(case)
    good = good_of(case, fx(case, "stage3")["good"])
    rounds = fx(case, "stage4")["rounds"]
    # the reference at one thread: marks visible at once, reads in file order
    for r in rounds:
        added = E.expand_pass(reads, K, pos, good, trim_quality=TRIM)
        assert added == r["added"], r["round"]
        assert good == good_of(case, r["good"]), r["round"]
    assert E.expand_loop(reads, K, pos, good_of(case, fx(case, "stage3")["good"]), trim_quality=TRIM)[1] == [r["added"] for r in rounds]
    # the engine's snapshot rounds: the same set once the closure is reached (test_reference_reached_the_closure)
    final, counts, _ = E.snapshot_rounds(E.candidate_reads(reads, K, TRIM), K, pos, good_of(case, fx(case, "stage3")["good"]),
                                         max_rounds=None, min_changed=1)
    assert final == good_of(case, rounds[-1]["good"])
    assert sum(counts) == sum(r["added"] for r in rounds)
    # and under the stopping rule the tool shares with the reference (fewer than 10 added ends the loop)
    assert E.snapshot_rounds(E.candidate_reads(reads, K, TRIM), K, pos, good_of(case, fx(case, "stage3")["good"]))[0] == final


# ---- stage 5: the read corrector and the printed files -----------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES)
def test_stage5_corrected_files(case):
    asc, pos, _ = ascending(case)
    good = good_of(case, fx(case, "stage4")["rounds"][-1]["good"])
    rc = R.ReadCorrector(pos, good, K)
    left, right = records(case)
    rows = [P.corrected_records(rc, recs, TRIM, True, OFFSET) for recs in (left, right)]
    streams = P.route_paired(*rows)
    s5 = fx(case, "stage5")
    base = [n[:-len(".fastq")] for n in C.case_texts(case)[2]]
    common = os.path.commonprefix(base)
    names = ["%s.00.0_0.cor.fastq" % base[0], "%s.00.0_0.cor.fastq" % base[1], "%s_unpaired.00.0_0.cor.fastq" % common,
             "%s.00.bad.fastq" % base[0], "%s.00.bad.fastq" % base[1]]
    assert sorted(s5["files"]) == sorted(names)
    for name, text in zip(names, streams):
        assert text == s5["files"][name], name
    assert rc.stats()[0] == s5["changed_reads"]
    assert "Changed %d bases in %d reads." % (rc.stats()[1], rc.stats()[0]) in s5["log"][0]
    assert "Failed to correct %d bases out of %d." % (rc.stats()[2], rc.stats()[3]) in s5["log"][1]


# ---- the drift guard -------------------------------------------------------------------------------------------------------------
def test_reference_binary_still_gives_the_committed_fixtures(tmp_path):
    from oracle import record_hammer_ref as Rec
    if not os.path.exists(Rec.BINARY):
        pytest.skip("oracle/_ref/hammer_ref is not built (no reference tree)")
    got = Rec.record(str(tmp_path))
    committed = sorted(f for f in os.listdir(C.FIXTURES) if f.endswith(".json.gz"))
    assert sorted(got) == committed
    for name in committed:
        with open(os.path.join(C.FIXTURES, name), "rb") as f:
            assert f.read() == got[name], name
