"""GPU: the read corrector (bbk_corrector_*, csrc/readcorrect.hip) and spades-kmerdata --correct against the restatement
(tests/readcorrect_restated.py).  Every comparison is an equality: every corrected read, every result flag, the four
counters, and where a read's searches ran -- on the device (1) exactly when the restatement's figures for the read are
inside bbk_corrector_limits(), through the host rule (2) exactly when they are not.  Sets are injected with
kmerset_from_device, bits with KMerSet.corrector(good)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build_host
from tests import readcorrect_cases as Cs
from tests import readcorrect_restated as R

pytestmark = pytest.mark.gpu

ERR_ARG = -1  # BBK_ERR_ARG of include/bbk.h
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def _set(ctx, keys, k):
    import torch
    d = torch.from_numpy(np.array(keys, dtype=np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    s = ctx.kmerset_from_device(d, len(keys), k)
    s._keep = d
    return s


def _expected(k, index, good, reads, limits):
    """(sequences, flags, where, the four counters, searches beyond the limits) by the restatement"""
    rc = R.ReadCorrector(index, good, k)
    out, res = rc.correct_batch(reads)
    searched = {r for r, _, _ in rc.searches}
    beyond = {r for r, _, inf in rc.searches if inf.max_heap > limits[0] or inf.pops > limits[1]}
    where = [2 if r in beyond else 1 if r in searched else 0 for r in range(len(reads))]
    n_beyond = sum(1 for _, _, inf in rc.searches if inf.max_heap > limits[0] or inf.pops > limits[1])
    return out, res, where, rc.stats(), n_beyond, rc


def _check(ctx, k, index, keys, good, reads):
    s = _set(ctx, keys, k)
    c = s.corrector(good)
    limits = c.limits()
    out, res, where, stats, n_beyond, rc = _expected(k, index, good, reads, limits)
    got_out, got_res, got_where = c.correct(reads)
    st = c.stats
    c.free()
    s.free()
    bad = [i for i in range(len(reads)) if got_out[i] != out[i]]
    assert not bad, (len(bad), bad[:5])
    assert got_res.tolist() == res
    assert got_where.tolist() == where
    assert [st[x] for x in B.Corrector.STATS] == stats + [n_beyond]
    return rc, where


@pytest.mark.parametrize("k", [11, 21, 32])
def test_island_edges(ctx, k):
    cases = Cs.island_cases(k)
    index, keys, good, reads = Cs.build_islands(k, cases)
    rc, where = _check(ctx, k, index, keys, good, reads)
    names = [c[0] for c in cases]
    assert where[names.index("every start good")] == 0 and where[names.index("shorter than k")] == 0
    assert where[names.index("two equal runs")] == 1


@pytest.mark.parametrize("k", [11, 21, 32])
def test_unit_cases_of_the_rule(ctx, k):
    """Every case with a search runs on the device, but the one that exists to outgrow size_thr = 100 * log2(n) + 1 > 100
    states: by the capacity rule that search belongs to the host path, and it is the case that shows the rule's other
    direction here."""
    cases = Cs.unit_cases(k) + [Cs.size_thr_case(k)]
    index, keys, good, reads = Cs.build(cases)
    reads += [("", []), (reads[0][0][:k - 1], reads[0][1][:k - 1])]
    rc, where = _check(ctx, k, index, keys, good, reads)
    searched = {r for r, _, _ in rc.searches}
    for i, c in enumerate(cases):
        assert where[i] == (0 if i not in searched else 2 if c.what == "size_thr" else 1), c.what
    assert len(searched) >= len(cases) - 3


def test_ties_on_the_device(ctx):
    """the crafted branching read at 60 bases: states of equal (penalty, pos) meet in the heaps, inside the limits"""
    k = 21
    read, qual, good_kmers = R.branching_read(k, 60, step=4)
    index, keys, good = R.make_index(good_kmers)
    s = _set(ctx, keys, k)
    c = s.corrector(good)
    limits = c.limits()
    c.free()
    s.free()
    rc = R.ReadCorrector(index, good, k)
    rc.correct_batch([(read, qual)])
    inf = rc.searches[0][2]
    assert inf.tie and 1 < inf.max_heap <= limits[0] and inf.pops <= limits[1]
    _, where = _check(ctx, k, index, keys, good, [(read, qual)])
    assert where == [1]


def test_overflow_goes_to_the_host_rule(ctx):
    """the same construction at 150 bases outgrows the heap; next to it reads that stay inside: where == 2 iff beyond"""
    k = 21
    big, qual, good_kmers = R.branching_read(k, 150, step=2)
    small, qual_s, good_s = R.branching_read(k, 60, step=4, seed=6)
    unit = [c for c in Cs.unit_cases(k) if c.what in ("both sides", "N corrected", "every start good")]
    index, keys, good = R.make_index(good_kmers | good_s | set().union(*[c.good for c in unit]))
    reads = [(big, qual), (small, qual_s)] + [(c.seq, c.qual) for c in unit] + [(big, qual)]
    rc, where = _check(ctx, k, index, keys, good, reads)
    assert where == [2, 1, 1, 1, 0, 2]
    assert max(inf.max_heap for _, _, inf in rc.searches) > 32


@pytest.fixture(scope="module")
def golden(golden_dir):
    k = 21
    index, keys, good, reads = Cs.golden_case(golden_dir, k)
    rc = R.ReadCorrector(index, good, k)
    out, res = rc.correct_batch(reads)
    return k, index, keys, good, reads, rc, out, res


def test_golden_reads_with_seeded_errors(ctx, golden, tmp_path):
    k, index, keys, good, reads, rc, out, res = golden
    assert len(reads) == 4108
    s = _set(ctx, keys, k)
    c = s.corrector(good)
    limits = c.limits()
    worst = (max(inf.max_heap for _, _, inf in rc.searches), max(inf.pops for _, _, inf in rc.searches))
    print("searches %d, largest heap %d, most pops %d, stats %r" % (len(rc.searches), worst[0], worst[1], rc.stats()))
    assert worst[0] <= limits[0] and worst[1] <= limits[1]
    got_out, got_res, got_where = c.correct(reads)
    assert got_out == out and got_res.tolist() == res
    st = c.stats
    assert [st[x] for x in B.Corrector.STATS] == rc.stats() + [0]
    searched = {r for r, _, _ in rc.searches}
    assert got_where.tolist() == [1 if r in searched else 0 for r in range(len(reads))]
    assert st["changed_reads"] > 1000 and st["uncorrected_nucleotides"] > 0
    c.free()
    s.free()
    # the same batch with every search through the host rule, in a process of its own
    np.save(str(tmp_path / "keys.npy"), np.array(keys, dtype=np.uint64))
    np.save(str(tmp_path / "good.npy"), np.array(good, dtype=np.uint8))
    with open(str(tmp_path / "reads.txt"), "w") as f:
        for seq, qual in reads:
            f.write("%s %s\n" % (seq, "".join(chr(q + 33) for q in qual)) if seq else "\n")
    env = dict(os.environ, BBK_CORRECTOR_HOST="1", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "readcorrect_child.py"), str(tmp_path), str(k)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(str(tmp_path / "out.txt")) as f:
        lines = f.read().split("\n")[:-1]
    assert lines[:len(reads)] == ["%d %s" % (res[i], out[i]) for i in range(len(reads))]
    host_stats = [int(x) for x in lines[len(reads)].split()]
    assert host_stats[:4] == rc.stats() and host_stats[4] == sum(1 for _, _, inf in rc.searches if inf.pops > 1 or inf.failed)
    assert lines[len(reads) + 1].split() == [str(2 if r in searched else 0) for r in range(len(reads))]


def test_batching(ctx, golden):
    """one call, and three calls over the reads in reversed order: the same reads, the same summed counters"""
    k, index, keys, good, reads, rc, out, res = golden
    n = 600
    sub = reads[:n]
    one = R.ReadCorrector(index, good, k)
    exp_out, exp_res = one.correct_batch(sub)
    s = _set(ctx, keys, k)
    c = s.corrector(good)
    got = c.correct(sub)
    assert got[0] == exp_out and got[1].tolist() == exp_res
    st1 = c.stats
    c.free()
    c = s.corrector(good)
    rev = sub[::-1]
    parts = [rev[:1], rev[1:257], rev[257:]]
    got_out, got_res = [], []
    for p in parts + [[]]:
        o, r_, _ = c.correct(p)
        got_out += o
        got_res += r_.tolist()
    assert got_out[::-1] == exp_out and got_res[::-1] == exp_res
    assert c.stats == st1 and [st1[x] for x in B.Corrector.STATS[:4]] == one.stats()
    c.free()
    s.free()


def test_from_expander(ctx):
    """Expander.corrector(): the bits of the expander as they are, copied"""
    k = 21
    c0 = [c for c in Cs.unit_cases(k) if c.what == "both sides"][0]
    index, keys, good, reads = Cs.build([c0])
    s = _set(ctx, keys, k)
    e = s.expander(good)
    c = e.corrector()
    e.free()
    out, res, where = c.correct(reads)
    assert out == [c0.corrected] and res.tolist() == [1] and where.tolist() == [1]
    assert c.stats == dict(changed_reads=1, changed_nucleotides=2, uncorrected_nucleotides=0,
                           total_nucleotides=len(c0.seq), host_searches=0)
    c.free()
    s.free()


def test_refusals(ctx):
    import ctypes as C
    L = B.load_library()
    k = 21
    c0 = [c for c in Cs.unit_cases(k) if c.what == "both sides"][0]
    index, keys, good, reads = Cs.build([c0])
    s = _set(ctx, keys, k)

    def refused(fn, match):
        with pytest.raises(B.BBKError, match=match) as err:
            fn()
        assert "bbk error %d:" % ERR_ARG in str(err.value)

    bad = np.array(good, dtype=np.uint8)
    bad[3] = 2
    refused(lambda: s.corrector(bad), "0 or 1")
    c = s.corrector(good)
    refused(lambda: c.correct([(c0.seq, [94] + c0.qual[1:])]), "93 at most")
    refused(lambda: c.correct([("A" * 65536, [30] * 65536)]), "65535 at most")
    assert c.stats["total_nucleotides"] == 0  # a refused call counts nothing
    # an expander with an open round, and one of another n
    e = s.expander(good)
    e.begin_round()
    refused(e.corrector, "a round is open")
    e.end_round()
    s2 = _set(ctx, keys[:-2], k)
    h = C.c_void_p()
    assert L.bbk_corrector_from_expander(ctx._h, s2._h, e._h, C.byref(h)) == ERR_ARG and not h.value
    assert b"the expander was made for" in L.bbk_last_error()
    # the sets the stage refuses
    rd = ctx.reads_from_ascii([c0.seq])
    canon = ctx.count(rd, k, B.CANONICAL)
    refused(lambda: canon.corrector(np.zeros(len(canon), dtype=np.uint8)), "both-strand")
    for x in (c, e, canon, rd, s2, s):
        x.free()


def test_cli(tmp_path, golden_dir):
    """spades-kmerdata --subcluster --expand --correct on a seeded mutated copy of the golden pair: the .cor.fastq and
    .bad.fastq of every input file are Read::print of the restatement run over the tool's own k-mers and good bits"""
    k = 21
    exe = [e for e in build_host.build() if e.endswith("spades-kmerdata")][0]
    files = []
    for i in (1, 2):
        reads = Cs.seeded_errors(Cs.golden_reads(golden_dir, (i,)), 0.01, 40 + i)
        p = str(tmp_path / ("in%d.fq" % i))
        with open(p, "w") as f:
            for j, (seq, qual) in enumerate(reads):
                # low qualities at both ends of some reads, so that both trims and the kept bad tail occur
                if j % 5 == 0:
                    qual = [2] * 3 + qual[3:-2] + [3, 1]
                elif j % 5 == 1:
                    qual = qual[:-4] + [2] * 4
                f.write("@r%d/%d extra words\n%s\n+\n%s\n" % (j, i, seq, "".join(chr(q + 33) for q in qual)))
        files.append(p)
    plain, prefix = str(tmp_path / "plain"), str(tmp_path / "out")
    common = ["-k", str(k), "-b", "100000"]
    r = subprocess.run([exe, "-o", plain, "--subcluster", "--expand"] + common + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Correction done" not in r.stdout + r.stderr
    r = subprocess.run([exe, "-o", prefix, "--subcluster", "--expand", "--correct"] + common + files, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    log = r.stdout + r.stderr
    exts = (".kmers", ".kmstat", ".hamming", ".hamming.idx", ".subclusters", ".subclusters.idx", ".newkmers")
    new = tuple(".%d.%s.fastq" % (i, w) for i in (0, 1) for w in ("cor", "bad"))
    assert sorted(os.listdir(str(tmp_path))) == sorted(["in1.fq", "in2.fq"] + ["plain" + e for e in exts] +
                                                       ["out" + e for e in exts + new])
    for e in exts:
        assert open(plain + e, "rb").read() == open(prefix + e, "rb").read(), e
    keys = np.fromfile(prefix + ".kmers", dtype=np.uint64)
    n = len(keys)
    rec = np.fromfile(prefix + ".kmstat", dtype=np.dtype([("c", "<u4"), ("tq", "<f4"), ("w", "<u8", (2,))]))
    good = (rec["c"][:n] & 1).astype(int).tolist()
    index = {"".join(R.NUCL[(int(x) >> (2 * i)) & 3] for i in range(k)): j for j, x in enumerate(keys)}
    rc = R.ReadCorrector(index, good, k)
    seen_trims = set()
    for i, p in enumerate(files):
        with open(p) as f:
            lines = f.read().split("\n")
        exp = {1: [], 0: []}
        recs = [(lines[j][1:], lines[j + 1], [ord(c) - 33 for c in lines[j + 3]]) for j in range(0, len(lines) - 3, 4)]
        trimmed = [R.trim_read(seq, qual, 4) for _, seq, qual in recs]
        out, res = rc.correct_batch([(t[0], t[1]) for t in trimmed])
        for (name, _, _), t, o, flag in zip(recs, trimmed, out, res):
            exp[flag].append(R.read_print(name, o, t[1], t[2], t[3], t[4], 33))
            seen_trims.add((t[2] > 0, t[3] < t[4]))
        assert open("%s.%d.cor.fastq" % (prefix, i)).read() == "".join(exp[1]), p
        assert open("%s.%d.bad.fastq" % (prefix, i)).read() == "".join(exp[0]), p
        assert exp[1] and exp[0]
    assert seen_trims == {(False, False), (True, False), (False, True), (True, True)}
    st = rc.stats()
    assert st[0] >= 1, "no read was changed: choose another seed or rate"
    assert "Correction done. Changed %d bases in %d reads." % (st[1], st[0]) in log
    assert "Failed to correct %d bases out of %d." % (st[2], st[3]) in log
    assert re.search(r"Searches corrected on the host: \d+", log)
