"""GPU: the expansion of the solid k-mers (bbk_expander_*, csrc/expand.hip) and spades-kmerdata --expand against the
restatement (tests/expander_restated.py).  Every comparison is by equality: the good bytes, the count of every round, the
status of every read.  Sets are injected with kmerset_from_device, bits with KMerSet.expander(good)."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build_host
from tests import expander_restated as E
from tests import kmerdata_restated as KR
from tests import subcluster_cases as Cs

pytestmark = pytest.mark.gpu

ERR_ARG = -1  # BBK_ERR_ARG of include/bbk.h
NO_LIMIT = 1000  # rounds: far more than any case here needs


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


def _closure(ctx, s, good, cands, **kw):
    e = s.expander(good)
    rd = ctx.reads_from_ascii(cands)
    counts = e.run(rd, **kw)
    out = e.export()
    assert e.good == int(out.sum())
    e.free()
    rd.free()
    return counts, out.tolist()


@pytest.mark.parametrize("k", [11, 21, 32])
def test_chain(ctx, k):
    reads, index, keys, good = E.chain_case(k)
    cands = E.candidate_reads(reads, k)
    closure, counts, states = E.snapshot_rounds(cands, k, index, good, None, 1)
    assert len(counts) >= 3 and counts == [9] + [6] * 9 + [4, 0] and sum(closure) == 98
    s = _set(ctx, keys, k)
    assert _closure(ctx, s, good, cands, max_rounds=NO_LIMIT, min_changed=1) == (counts, closure)
    # the reference's stop rule: 9 < 10 ends the run after its first round, with G_1
    g1, c1, _ = E.snapshot_rounds(cands, k, index, good)
    assert c1 == [9] and g1 == states[1]
    assert _closure(ctx, s, good, cands) == (c1, g1)
    assert _closure(ctx, s, good, cands, max_rounds=2, min_changed=1) == (counts[:2], states[2])
    # the same rounds through begin / push / end: three pushes per round, the reads in reversed order
    e = s.expander(good)
    assert e.good == 31
    rev = cands[::-1]
    parts = [ctx.reads_from_ascii(rev[a:b]) for a, b in ((0, 7), (7, 8), (8, 30))]
    got = []
    for r in range(len(counts)):
        e.begin_round()
        for p in parts:
            assert e.push(p) is None
        got.append(e.end_round())
        assert e.export().tolist() == states[r + 1]
        assert e.good == sum(states[r + 1])
    assert got == counts
    for h in parts + [e, s]:
        h.free()


def _edge_cases(k, rng):
    """[(what, read, good starts, absent starts, expected status)]: one crafted read each.  `absent`: starts whose k-mer
    is left out of the set."""
    def bases(n):
        return "".join(rng.choice(list("ACGT"), n))

    def read(nk):
        return bases(nk + k - 1)

    def every(nk, step):
        return sorted(set(range(0, nk, step)) | {nk - 1})

    out = [("length k, good", read(1), [0], [], 2),
           ("length k, not good", read(1), [], [], 0),
           ("gap k", read(k + 1), [0, k], [], 1),
           ("gap k + 1", read(k + 2), [0, k + 1], [], 0),
           ("start 0 not good", read(40), list(range(1, 40)), [], 0),
           ("last start not good", read(40), list(range(0, 39)), [], 0),
           ("all good", read(70), list(range(70)), [], 2),
           ("300 bases", read(300 - k + 1), every(300 - k + 1, k - 1), [], 1),
           ("300 bases, a gap of k + 1 beyond start 256", read(300 - k + 1),
            [p for p in range(300 - k + 1) if not 257 <= p <= 257 + k - 1], [], 0),
           ("300 bases, all good but one beyond start 256", read(300 - k + 1),
            [p for p in range(300 - k + 1) if p != 270], [], 1)]
    for nk in (64, 65, 128, 129):
        out.append(("nk = %d" % nk, read(nk), every(nk, k), [], 1))
        out.append(("nk = %d, only the last start missing" % nk, read(nk), list(range(nk - 1)), [], 0))
        out.append(("nk = %d, all good" % nk, read(nk), list(range(nk)), [], 2))
    # a run of non-good starts across the boundary between the chunks of 64 starts
    out.append(("run of k - 1 across starts 63 | 64", read(129), [p for p in range(129) if not 54 <= p < 54 + k - 1], [], 1))
    out.append(("run of k across starts 63 | 64", read(129), [p for p in range(129) if not 54 <= p < 54 + k], [], 0))
    out.append(("run of k ending at start 63", read(129), [p for p in range(129) if not 64 - k <= p < 64], [], 0))
    out.append(("run of k from start 64", read(129), [p for p in range(129) if not 64 <= p < 64 + k], [], 0))
    out.append(("run of k across starts 127 | 128", read(140), [p for p in range(140) if not 120 <= p < 120 + k], [], 0))
    out.append(("few good starts, none more than k apart", read(140), [0, 20, 40, 61, 82, 103, 124, 139], [], 1))
    out.append(("a chunk without a good start", read(140), list(range(64)) + list(range(128, 140)), [], 0))
    # a k-mer that is not in the set
    out.append(("absent in the middle, covered", read(40), [0, 19, 39], [20], 1))
    out.append(("absent in the middle, its good neighbours k + 1 apart", read(60), [0, 19, 19 + k + 1, 59], [20], 0))
    out.append(("absent at start 0", read(40), list(range(1, 40)), [0], 0))
    out.append(("shorter than k", bases(k - 1), [], [], 0))
    # the same k-mer twice in one read: starts 0 .. 19 again at 40 .. 59
    r = bases(40)
    out.append(("a k-mer twice in one read", r + r, [0, 19, 40, 59], [], 1))
    # two reads solid in the same round that share the starts 10 .. 29 of t
    t = bases(60 + k - 1)
    out.append(("two reads, first", t[:30 + k - 1], [0, 10, 20, 29], [], 1))
    out.append(("two reads, second", t[10:40 + k - 1], [0, 10, 19, 29], [], 1))
    return out


def test_edges_of_the_solid_test(ctx):
    k = 21
    cases = _edge_cases(k, np.random.default_rng(21))
    kmers, good_kmers = set(), set()
    for what, read, good_starts, absent, _ in cases:
        nk = max(len(read) - k + 1, 0)
        assert all(0 <= p < nk for p in good_starts + absent) and not set(good_starts) & set(absent), what
        kmers.update(read[p:p + k] for p in range(nk) if p not in absent)
        good_kmers.update(read[p:p + k] for p in good_starts)
    assert not kmers & {read[p:p + k] for _, read, _, absent, _ in cases for p in absent}
    index, keys = E.both_strand_index(kmers)
    assert len(keys) == 2 * len(kmers)  # no k-mer is another's reverse complement
    good = [0] * len(keys)
    for x in good_kmers:
        good[index[x]] = 1
    # the reverse complements of some k-mers that will be marked are good from the start, the others are not: both stay
    rc_good = sorted(kmers - good_kmers)[::3]
    for x in rc_good:
        good[index[KR.revcomp(x)]] = 1
    cands = [read for _, read, _, _, _ in cases]
    nxt, changed, status = E.snapshot_round(cands, k, index, good)
    assert status == [st for _, _, _, _, st in cases], [c[0] for c, s in zip(cases, status) if c[4] != s]
    for what, read, good_starts, absent, st in cases:  # the starts as given are what the restatement sees
        nk = max(len(read) - k + 1, 0)
        if what.startswith(("a k-mer twice", "two reads")):
            continue
        assert [p for p in range(nk) if p not in absent and good[index[read[p:p + k]]]] == sorted(good_starts), what
    assert changed > 0
    s = _set(ctx, keys, k)
    e = s.expander(good)
    rd = ctx.reads_from_ascii(cands)
    empty = ctx.reads_from_ascii([])
    e.begin_round()
    assert e.push(empty, status=True).tolist() == [] and e.push(empty) is None
    assert e.push(rd, status=True).tolist() == status
    assert e.export().tolist() == good  # G_r stands until the round ends
    assert e.end_round() == changed
    got = e.export().tolist()
    assert got == nxt
    twice = cases[[c[0] for c in cases].index("a k-mer twice in one read")][1]
    assert sum(nxt[index[twice[p:p + k]]] for p in range(20)) == 20  # both occurrences, counted once in `changed`
    for x in kmers:  # no reverse complement was touched
        assert got[index[KR.revcomp(x)]] == good[index[KR.revcomp(x)]]
    # on to the closure, the statuses of every round included
    cur = nxt
    while True:
        nxt, changed, status = E.snapshot_round(cands, k, index, cur)
        e.begin_round()
        assert e.push(rd, status=True).tolist() == status
        assert e.end_round() == changed and e.export().tolist() == nxt
        cur = nxt
        if changed == 0:
            break
    assert 2 in status and 0 in status
    for h in (e, rd, empty, s):
        h.free()


def test_golden_reads(ctx, golden_dir):
    k = 21
    with gzip.open(os.path.join(golden_dir, "ecoli_1K_1.fq.gz"), "rt") as f:
        lines = f.read().split("\n")
    reads = [(lines[i + 1], [ord(c) - 33 for c in lines[i + 3]]) for i in range(0, len(lines) - 3, 4)]
    cands = E.candidate_reads(reads, k)
    assert len(cands) == 2054
    rd = ctx.reads_from_ascii(cands)
    s = ctx.count(rd, k, B.BOTH_STRANDS)
    index, keys = E.both_strand_index({c[p:p + k] for c in cands for p in range(len(c) - k + 1)})
    assert s.export()[:, 0].tolist() == keys
    good = [int(x) for x in np.random.default_rng(2101).random(len(keys)) < 0.5]
    closure, counts, _ = E.snapshot_rounds(cands, k, index, good, None, 1)
    assert len(counts) >= 2 and counts[0] > 0 and counts[-1] == 0
    e = s.expander(good)
    assert e.run(rd, max_rounds=NO_LIMIT, min_changed=1) == counts
    assert e.export().tolist() == closure and e.good == sum(closure)
    for h in (e, s, rd):
        h.free()


def test_store(ctx, tmp_path):
    """the bits go back into the subclusters: the first n only, and nothing else moves.  The case is the one whose
    consensus is a new k-mer; next to its cluster the set holds the k-mers of one read, singletons whose total_qual makes
    some of them good"""
    from tests.test_gpu_subcluster import _load, _write_case
    k = 21
    chain = Cs.chain_case(k)
    rng = np.random.default_rng(77)
    read = "".join(rng.choice(list("ACGT"), 40 + k - 1))
    items = [(int(x), int(c), t, q) for x, c, t, q in zip(chain["keys"], chain["count"], chain["tq"], chain["quals"])]
    good_starts = {0, 15, 30, 39}
    for p in range(40):
        items.append((KR.kmer_key(read[p:p + k]), 20, np.float32(1e-4 if p in good_starts else 0.5), [30] * k))
    case = Cs.make_case(k, items, [list(range(5))])
    exp = Cs.restate(case)
    n = len(case["keys"])
    assert len(exp["new_keys"]) == 1 and len(exp["good"]) == n + 1
    index = {KR.kmer_key(read[p:p + k]): case["keys"].index(KR.kmer_key(read[p:p + k])) for p in range(40)}
    assert sorted(p for p in range(40) if exp["good"][index[KR.kmer_key(read[p:p + k])]]) == sorted(good_starts)
    _write_case(case, str(tmp_path / "c"))
    s, ks, hc = _load(ctx, str(tmp_path / "c"), k)
    sc = hc.subcluster(ks)
    before = sc.export()
    assert before["good"].tolist() == exp["good"].tolist()
    e = sc.expander()
    assert e.export().tolist() == before["good"][:n].tolist()
    rd = ctx.reads_from_ascii([read])
    assert e.run(rd, min_changed=1) == [36, 0]
    e.store(sc)
    after = sc.export()
    assert after["good"][:n].tolist() == e.export().tolist() and int(after["good"][:n].sum()) == int(before["good"][:n].sum()) + 36
    assert after["good"][n:].tolist() == before["good"][n:].tolist()
    for f in ("members", "sizes", "per_cluster", "new_keys", "bic", "errs", "stats"):
        assert after[f].tobytes() == before[f].tobytes(), f
    sc.write(str(tmp_path / "w"))
    rec = np.fromfile(str(tmp_path / "w.kmstat"), dtype=np.dtype([("c", "<u4"), ("tq", "<f4"), ("w", "<u8", (2,))]))
    assert (rec["c"] & 1).astype(np.uint8).tolist() == after["good"].tolist()
    for h in (e, rd, sc, hc, ks, s):
        h.free()


def test_refusals(ctx):
    import ctypes as C
    L = B.load_library()
    k = 21
    reads, index, keys, good = E.chain_case(k)
    s = _set(ctx, keys, k)
    rd = ctx.reads_from_ascii([r for r, _ in reads])

    def refused(fn, match):
        with pytest.raises(B.BBKError, match=match) as err:
            fn()
        assert "bbk error %d:" % ERR_ARG in str(err.value)

    bad = np.array(good, dtype=np.uint8)
    bad[5] = 2
    refused(lambda: s.expander(bad), "0 or 1")
    e = s.expander(good)
    refused(lambda: e.push(rd), "no round is open")
    refused(e.end_round, "no round is open")
    refused(lambda: e.run(rd, max_rounds=0), "max_rounds is 0")
    e.begin_round()
    refused(e.begin_round, "a round is open")
    refused(lambda: e.run(rd), "a round is open")
    assert e.end_round() == 0  # nothing was pushed
    assert e.run(rd) == [9]
    # a set and subclusters of different n
    case = Cs.chain_case(k)
    from tests.test_gpu_subcluster import _load, _write_case
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        _write_case(case, os.path.join(d, "c"))
        s2, ks2, hc2 = _load(ctx, os.path.join(d, "c"), k)
    sc2 = hc2.subcluster(ks2)
    assert len(s2) != len(s)
    h = C.c_void_p()
    assert L.bbk_expander_from_subclusters(ctx._h, s._h, sc2._h, C.byref(h)) == ERR_ARG and not h.value
    assert b"the set has" in L.bbk_last_error()
    refused(lambda: e.store(sc2), "the expander holds")
    # the sets the stage refuses
    canon = ctx.count(rd, k, B.CANONICAL)
    refused(lambda: canon.expander(np.zeros(len(canon), dtype=np.uint8)), "both-strand")
    for x in (e, sc2, hc2, ks2, s2, canon, rd, s):
        x.free()


def test_cli(tmp_path, golden_dir):
    """spades-kmerdata --subcluster with and without --expand on the golden pair.  At the thresholds of config.info every
    k-mer of these error-free reads that a read could make good is good already (the CPU restatements give 1964 good of
    1974, and no round adds one).  With --singleton-threshold 0.99999995 --no-correct-threshold a k-mer is good only when
    the float 1 - total_qual is exactly 1: the restatements then leave a handful more k-mers bad, and the expansion adds
    at least one of them."""
    k = 21
    exe = [e for e in build_host.build() if e.endswith("spades-kmerdata")][0]
    files = [os.path.join(golden_dir, "ecoli_1K_%d.fq.gz" % i) for i in (1, 2)]
    common = ["-k", str(k), "-b", "60000", "--singleton-threshold", "0.99999995", "--no-correct-threshold"]
    plain, prefix = str(tmp_path / "plain"), str(tmp_path / "out")
    r = subprocess.run([exe, "-o", plain, "--subcluster"] + common + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Solid k-mers" not in r.stdout + r.stderr
    r = subprocess.run([exe, "-o", prefix, "--subcluster", "--expand", "--expand-min-changed", "1"] + common + files,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    log = r.stdout + r.stderr
    exts = (".kmers", ".kmstat", ".hamming", ".hamming.idx", ".subclusters", ".subclusters.idx", ".newkmers")
    assert sorted(os.listdir(str(tmp_path))) == sorted(p + e for p in ("plain", "out") for e in exts)
    for e in exts:
        if e != ".kmstat":
            assert open(plain + e, "rb").read() == open(prefix + e, "rb").read(), e
    dt = np.dtype([("c", "<u4"), ("tq", "<f4"), ("w", "<u8", (2,))])
    a, b = np.fromfile(plain + ".kmstat", dtype=dt), np.fromfile(prefix + ".kmstat", dtype=dt)
    assert len(a) == len(b)
    assert (a["c"] >> 1).tolist() == (b["c"] >> 1).tolist() and a["tq"].tobytes() == b["tq"].tobytes()
    assert a["w"].tobytes() == b["w"].tobytes()
    # the restatement's snapshot rounds from the bits of the --subcluster run
    keys = np.fromfile(plain + ".kmers", dtype=np.uint64)
    n = len(keys)
    reads = []
    for p in files:
        with gzip.open(p, "rt") as f:
            lines = f.read().split("\n")
        reads += [(lines[i + 1], [ord(c) - 33 for c in lines[i + 3]]) for i in range(0, len(lines) - 3, 4)]
    index, rkeys = E.index_of_reads(reads, k)
    assert rkeys == keys.tolist()
    good = (a["c"][:n] & 1).astype(int).tolist()
    closure, counts, _ = E.snapshot_rounds(E.candidate_reads(reads, k), k, index, good, 25, 1)
    assert sum(counts) >= 1, "nothing expands at these thresholds: choose others"
    assert (b["c"][:n] & 1).astype(int).tolist() == closure
    assert (b["c"][n:] & 1).tolist() == (a["c"][n:] & 1).tolist()
    got = [(int(i), int(c)) for i, c in re.findall(r"Solid k-mers iteration (\d+) produced (\d+) new k-mers\.", log)]
    assert got == list(enumerate(counts))
    assert log.count("Solid k-mers finalized") == 1
    # the iteration limit
    r = subprocess.run([exe, "-o", str(tmp_path / "one"), "--expand", "--expand-min-changed", "0",
                        "--expand-max-iterations", "1"] + common + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.findall(r"iteration (\d+) produced (\d+)", r.stdout + r.stderr) == [("0", str(counts[0]))]
