"""GPU: the prepared read batch (bbk_hreads_*, csrc/hreads.hip), its views, bbk_corrector_correct_prepared and
spades-kmerdata --resident-bytes.  Every comparison is an equality: trims, both stretch tables and the candidate flags
against the literal restatements (tests/kmerdata_restated.py through tests/hreads_restated.py), and everything pushed
from a view against the same thing pushed from host-cut strings."""
import os
import subprocess
import sys

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build_host
from tests import expander_restated as ER
from tests import hreads_restated as HR
from tests.hreads_child import arrays, compare_corrections, device_set, golden_inputs
from tests import kmerdata_restated as KR
from tests import readcorrect_cases as Cs

pytestmark = pytest.mark.gpu

ERR_ARG = -1  # BBK_ERR_ARG of include/bbk.h
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def tables_of(hr):
    """what the batch holds, in the shape of HR.prepare"""
    trims = [tuple(int(x) for x in t) for t in hr.trims()]
    out = []
    for table in ("kmer", "corrector"):
        off, st = hr.stretches(table)
        out.append([[tuple(int(x) for x in st[j]) for j in range(int(off[i]), int(off[i + 1]))] for i in range(len(hr))])
    return trims, out[0], out[1], hr.candidates().tolist()


def check_batch(ctx, records, k, tq, trim=HR.literal_trim):
    """trim: the rule the batch's trims must follow (HR.identity_trim for tq = B.NO_TRIM)"""
    want = HR.prepare(records, k, tq, trim=trim)
    hr = ctx.hammer_reads(*arrays(records), k, trim_quality=tq)
    got = tables_of(hr)
    L = hr._L
    counts = (len(hr), L.bbk_hreads_kmer_stretches(hr._h), L.bbk_hreads_corrector_stretches(hr._h), L.bbk_hreads_candidates(hr._h))
    hr.free()
    for name, g, w in zip(("trims", "k-mer table", "corrector table", "candidates"), got, want):
        bad = [i for i in range(len(records)) if g[i] != w[i]]
        assert not bad, (name, k, tq, len(bad), [(i, records[i], g[i], w[i]) for i in bad[:3]])
    assert counts == (len(records), sum(len(x) for x in want[1]), sum(len(x) for x in want[2]), sum(want[3]))
    return want


def with_empties(records):
    m = len(records) // 2
    return [("", [])] + records[:m] + [("", []), ("", [])] + records[m:] + [("", [])]


def crafted(k):
    rng = np.random.default_rng(200 + k)
    recs = [(s, q) for _, s, q in KR.crafted_reads(k, rng)]
    recs += [(s.lower(), q) for s, q in recs[:8]] + [(s.replace("N", "."), q) for s, q in recs[4:8]]
    recs += [(s[:3] + s[3:9].lower() + s[9:], q) for s, q in recs[:8]]
    rb = "".join(rng.choice(list("ACGT"), k + 1))
    return recs + [(rb[:n], [30] * n) for n in (k - 1, k, k + 1)]


@pytest.mark.parametrize("k", [5, 21, 32])
def test_crafted_reads(ctx, k):
    recs = crafted(k)
    want = check_batch(ctx, with_empties(recs), k, 4)
    assert any(len(x) > 1 for x in want[1]) and any(a != b for a, b in zip(want[1], want[2]))  # the tables do differ
    check_batch(ctx, with_empties(recs), k, 0)


@pytest.mark.parametrize("k", [5, 21, 32])
def test_records_taken_as_trimmed(ctx, k):
    """trim_quality = B.NO_TRIM: every trim is (0, n) -- (0, 0) for an empty record -- and the tables and the flag are
    those of a trimmed read of these bases.  The restatement alone says that the boundary records tell this from a trim
    at quality 4: in the trims, in the corrector table (in record coordinates) and in the candidate flag."""
    recs = HR.boundary_records(np.random.default_rng(9))
    assert len(recs) == 512
    at4, whole = HR.prepare(recs, k, 4), HR.prepare(recs, k, None, trim=HR.identity_trim)
    assert sum(t != (0, len(s)) for t, (s, _) in zip(at4[0], recs)) >= 300
    assert sum([(a + t[0], n) for a, n in x] != y for t, x, y in zip(at4[0], at4[2], whole[2])) >= 50
    assert sum(a != b for a, b in zip(at4[3], whole[3])) >= 100
    want = check_batch(ctx, with_empties(recs), k, B.NO_TRIM, trim=HR.identity_trim)
    assert want[0][0] == (0, 0) and want[0][1] == (0, len(recs[0][0]))  # an empty record; the first boundary record
    check_batch(ctx, with_empties(crafted(k)), k, B.NO_TRIM, trim=HR.identity_trim)


@pytest.mark.parametrize("k,tq", [(21, 4), (21, 0), (5, 4), (5, 0), (32, 1)])
def test_events_at_chunk_boundaries(ctx, k, tq):
    recs = HR.boundary_records(np.random.default_rng(9))
    want = check_batch(ctx, with_empties(recs), k, tq)
    assert sum(want[3]) > 20 and sum(len(x) == 2 for x in want[1]) > 20


@pytest.fixture(scope="module")
def random_batch():
    rng = np.random.default_rng(77)
    return with_empties(HR.random_records(rng, 2000, max_len=300, odd=0.02) + HR.random_records(rng, 200, max_len=300))


def test_random_records(ctx, random_batch):
    want = check_batch(ctx, random_batch, 21, 4)
    assert 300 < sum(want[3]) < len(random_batch) and max(len(x) for x in want[1]) >= 3


def test_views(ctx, random_batch):
    """The stretch view is the upper-cased stretch substrings; its qualities are the ranges (held through the k-mer
    statistics, whose per-position quality sums move with any shift: the library exports no qualities).  The candidate
    view is expander_restated.candidate_reads."""
    k = 21
    recs = random_batch
    _, kst, _, _ = HR.prepare(recs, k, 4)
    hr = ctx.hammer_reads(*arrays(recs), k)
    reads, quals = hr.stretch_view()
    want = [(s[a:a + n].upper(), q[a:a + n]) for (s, q), st in zip(recs, kst) for a, n in st]
    assert reads.to_list() == [s for s, _ in want] and reads.bases == sum(len(s) for s, _ in want)
    assert hr.stretch_view()[0]._h.value == reads._h.value  # cached
    cand = hr.candidate_view()
    assert cand.to_list() == ER.candidate_reads(recs, k)
    # the statistics from the view and from host-cut strings
    host = ctx.reads_from_ascii([s for s, _ in want])
    hq = ctx.quals(host, *arrays(want)[1:])
    kset = ctx.count(host, k, B.BOTH_STRANDS)
    a, b = kset.kmer_stats(), kset.kmer_stats()
    a.push(host, hq)
    b.push(reads, quals)
    a.finish()
    b.finish()
    for x, y in zip(a.export(), b.export()):
        assert np.array_equal(x, y)
    assert int(a.export()[0].sum()) == 2 * sum(len(s) - k + 1 for s, _ in want)
    reads.free()  # borrowed: frees nothing
    assert hr.stretch_view()[0].to_list()[:3] == [s for s, _ in want[:3]]
    for x in (a, b, kset, hq, host, hr):
        x.free()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return golden_inputs(golden_dir)


def test_same_bytes_from_the_views(ctx, golden_dir):
    """the golden pair at k = 21: set, KMerStat export and expansion from the views equal the host-cut path"""
    k = 21
    recs = Cs.golden_reads(golden_dir)
    assert len(recs) == 2 * 2054
    _, kst, _, cand = HR.prepare(recs, k, 4)
    cut = [(s[a:a + n], q[a:a + n]) for (s, q), st in zip(recs, kst) for a, n in st]
    hr = ctx.hammer_reads(*arrays(recs), k)
    reads, quals = hr.stretch_view()
    c1, c2 = ctx.counter(k, B.BOTH_STRANDS), ctx.counter(k, B.BOTH_STRANDS)
    c1.push_ascii([s for s, _ in cut])
    c2.push(reads)
    s1, s2 = c1.finish(), c2.finish()
    assert np.array_equal(s1.export(), s2.export()) and len(s1) > 1000  # a 1 kb region, both strands
    host = ctx.reads_from_ascii([s for s, _ in cut])
    hq = ctx.quals(host, *arrays(cut)[1:])
    a, b = s1.kmer_stats(), s1.kmer_stats()
    a.push(host, hq)
    b.push(reads, quals)
    a.finish()
    b.finish()
    ea, eb = a.export(), b.export()
    for x, y in zip(ea, eb):
        assert np.array_equal(x, y)
    # the expansion: two thirds of the k-mers seen twice start good, so that solid reads have k-mers left to mark
    good0 = ((ea[0] >= 2) & (np.arange(len(s1)) % 3 != 0)).astype(np.uint8)
    cand_host = ctx.reads_from_ascii([recs[i][0][t0:t0 + tl] for i, (t0, tl) in enumerate(HR.prepare(recs, k, 4)[0]) if cand[i]])
    e1, e2 = s1.expander(good0), s1.expander(good0)
    r1, r2 = e1.run(cand_host, max_rounds=5, min_changed=1), e2.run(hr.candidate_view(), max_rounds=5, min_changed=1)
    assert r1 == r2 and r1[0] > 0 and np.array_equal(e1.export(), e2.export())
    for x in (e1, e2, cand_host, a, b, hq, host, s1, s2, hr):
        x.free()


def test_correct_prepared(ctx, golden):
    st, wh = compare_corrections(ctx, golden)
    assert st["changed_reads"] > 1000 and st["host_searches"] == 0 and wh == [0, 1]
    # the host-array entry is the prepared one over a batch that is taken as trimmed already
    k, keys, good, trimmed, _ = golden
    s = device_set(ctx, keys, k)
    c1, c2 = s.corrector(good), s.corrector(good)
    bases, quals, off = arrays(trimmed)
    out1, res1, where1 = c1.correct_arrays(bases, quals, off)
    hr = ctx.hammer_reads(bases, quals, off, k, trim_quality=B.NO_TRIM)
    out2, off2, res2, where2 = c2.correct_prepared(hr)
    assert np.array_equal(off, off2) and np.array_equal(out1, out2)
    assert np.array_equal(res1, res2) and np.array_equal(where1, where2) and c1.stats == c2.stats == st
    for x in (hr, c1, c2, s):
        x.free()


def test_print_of_records_taken_as_trimmed(ctx):
    """a B.NO_TRIM batch through correct_resident and Corrected.print: no ltrim= / rtrim=, no padding, the bad ends and
    the Ns of the records stay where they are -- the text of tests/readprint_restated.py with the identity trim"""
    from tests import readcorrect_restated as R
    from tests import readprint_restated as P
    from tests.readprint_child import run_batch
    from tests.test_gpu_readprint import shape_cases
    k = 21
    index, keys, good, recs = shape_cases(k)
    rows = P.corrected_records(R.ReadCorrector(index, good, k), recs, None, True, 33)
    want = [x.encode("latin-1") for x in P.route_single(rows)]
    got = run_batch(ctx, k, keys, good, recs, trim_quality=B.NO_TRIM)
    assert got["streams"] == want and all(len(w) > 0 for w in want)
    assert b"trim=" not in want[0] + want[1] and {x[2] for x in rows} >= {P.NONE, P.OK, P.CHANGED}
    assert got["sides"][0][4] == [x[3] for x in rows] and got["sides"][0][5] == [x[2] for x in rows]
    at4 = P.corrected_records(R.ReadCorrector(index, good, k), recs, 4, True, 33)
    assert sum(a[1] != b[1] for a, b in zip(rows, at4)) >= 10  # the same records do print differently when trimmed at 4


def test_correct_prepared_by_the_host_rule(golden_dir):
    """the same comparison with every search through the host rule (BBK_CORRECTOR_HOST=1), in a process of its own"""
    env = dict(os.environ, BBK_CORRECTOR_HOST="1", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "hreads_child.py"), golden_dir], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0 and "host searches" in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split("host searches")[1].split()[0]) > 1000


def test_refusals(ctx, golden):
    k, keys, good, trimmed, raw = golden

    def refused(fn, match):
        with pytest.raises(B.BBKError, match=match) as err:
            fn()
        assert "bbk error %d:" % ERR_ARG in str(err.value)

    seq = "ACGTTGCA" * 5
    one = ([(seq, [30] * len(seq))])
    refused(lambda: ctx.hammer_reads(*arrays([(seq, [94] + [30] * (len(seq) - 1))]), 21), "93 at most")
    b, q, off = arrays(one * 2)
    refused(lambda: ctx.hammer_reads(b, q, np.array([0, len(seq), 5], dtype=np.uint64), 21), "descend")
    refused(lambda: ctx.hammer_reads(b, q, off, 0), "1 <= k <= 32")
    refused(lambda: ctx.hammer_reads(b, q, off, 33), "1 <= k <= 32")
    s = device_set(ctx, keys, k)
    c = s.corrector(good)
    hr = ctx.hammer_reads(b, q, off, 20)
    refused(lambda: c.correct_prepared(hr), "prepared for k = 20")
    hr.free()
    long_ = ctx.hammer_reads(*arrays([("A" * 65536, [30] * 65536)]), k)  # from_host takes it ...
    assert long_.trims().tolist() == [[0, 65536]] and long_.candidates().tolist() == [1]
    refused(lambda: c.correct_prepared(long_), "65535 at most")        # ... correct_prepared does not
    assert c.stats["total_nucleotides"] == 0
    empty = ctx.hammer_reads(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64), k)
    assert len(empty) == 0 and len(empty.candidate_view()) == 0 and len(empty.stretch_view()[0]) == 0
    out, off2, res, where = c.correct_prepared(empty)
    assert len(out) == 0 and off2.tolist() == [0] and len(res) == 0
    for x in (empty, long_, c, s):
        x.free()


def test_cli_resident_bytes(tmp_path, golden_dir):
    """spades-kmerdata --correct in several blocks: every output file is the same bytes with --resident-bytes 0, with a
    budget larger than the input, and with one that covers the first block only"""
    k = 21
    exe = [e for e in build_host.build() if e.endswith("spades-kmerdata")][0]
    files = []
    for i in (1, 2):
        reads = Cs.seeded_errors(Cs.golden_reads(golden_dir, (i,)), 0.01, 40 + i)
        p = str(tmp_path / ("in%d.fq" % i))
        with open(p, "w") as f:
            for j, (seq, qual) in enumerate(reads):
                if j % 5 == 0:
                    qual = [2] * 3 + qual[3:-2] + [3, 1]
                elif j % 5 == 1:
                    qual = qual[:-4] + [2] * 4
                f.write("@r%d/%d extra words\n%s\n+\n%s\n" % (j, i, seq, "".join(chr(q + 33) for q in qual)))
        files.append(p)
    exts = (".kmers", ".kmstat", ".hamming", ".hamming.idx", ".subclusters", ".subclusters.idx", ".newkmers") + \
        tuple(".%d.%s.fastq" % (i, w) for i in (0, 1) for w in ("cor", "bad"))
    outs = {}
    for name, budget in (("zero", "0"), ("all", "100000000"), ("first", "130000")):
        prefix = str(tmp_path / name)
        r = subprocess.run([exe, "-o", prefix, "--correct", "-k", str(k), "-b", "60000", "--resident-bytes", budget] + files,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Correction done" in r.stdout + r.stderr
        outs[name] = {e: open(prefix + e, "rb").read() for e in exts}
    assert all(len(outs["zero"][e]) > 0 for e in exts if e != ".newkmers")  # the subclustering may add no k-mer
    for name in ("all", "first"):
        for e in exts:
            assert outs[name][e] == outs["zero"][e], (name, e)
