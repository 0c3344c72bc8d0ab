"""GPU: BayesHammer's Bayesian subclustering (bbk_hamclusters_subcluster, csrc/subclust.hip) and spades-kmerdata
--subcluster against the literal restatement (tests/subcluster_restated.py).  Every export is compared by equality, the
BIC of every cluster through its bits.  Clusters are injected with bbk_kmerstats_load / bbk_hamclusters_load unless a
test says otherwise.

With `loglik += count * logL` contracted into a fused multiply-add, the `count_ties` case fails at k = 21 and at k = 32:
the BIC of one of its clusters gets other bits (tests/test_subcluster_restated.py::test_fused_multiply_add_changes_a_bic
shows that on the CPU, with an exactly rounded a * b + c).  For the device's own log in place of the host's std::log no
failing case is known: it would change a BIC only for a cluster total whose two logarithms differ in the last place, the
device's log cannot be evaluated without running it, and no such total has been looked for.  What keeps it out is the
build: the code object of subclust.hip holds no log instruction and calls no log routine."""
import gzip
import hashlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build_host
from tests import kmerdata_restated as KR
from tests import subcluster_cases as Cs
from tests import subcluster_restated as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1  # BBK_ERR_ARG of include/bbk.h
FIELDS = ("good", "members", "sizes", "per_cluster", "new_keys", "errs", "stats")


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def _write_case(case, prefix, cluster_order=None):
    """<prefix>.keys.npy, <prefix>.kmstat, <prefix>.hamming(.idx) of a case"""
    n, k = len(case["keys"]), case["k"]
    np.save(prefix + ".keys.npy", np.array(case["keys"], dtype=np.uint64))
    rec = np.zeros(n, dtype=np.dtype([("c", "<u4"), ("tq", "<f4"), ("w", "<u8", ((6 * k + 63) // 64,))]))
    rec["c"], rec["tq"], rec["w"] = case["count"] << 1, case["tq"], case["qual_words"]
    rec.tofile(prefix + ".kmstat")
    sizes = [int(s) for s in case["sizes"]]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    order = list(range(len(sizes))) if cluster_order is None else list(cluster_order)
    mem = [case["members"][starts[c]:starts[c + 1]] for c in order]
    (np.concatenate(mem) if mem else np.zeros(0)).astype(np.uint64).tofile(prefix + ".hamming")
    np.array([sizes[c] for c in order], dtype=np.uint64).tofile(prefix + ".hamming.idx")


def _load(ctx, prefix, k):
    import torch
    keys = np.load(prefix + ".keys.npy")
    d = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    s = ctx.kmerset_from_device(d, len(keys), k)
    s._keep = d
    return s, ctx.kmerstats_load(s, prefix + ".kmstat"), ctx.hamclusters_load(len(keys), prefix + ".hamming")


def _run(ctx, case, tmp_path, name, params=None, cluster_order=None):
    prefix = str(tmp_path / name)
    _write_case(case, prefix, cluster_order)
    s, ks, hc = _load(ctx, prefix, case["k"])
    sc = hc.subcluster(ks, **(params or {}))
    got = sc.export()
    got["host_kmers"], got["count"], got["new"] = sc.host_kmers, len(sc), sc.new_kmers
    for h in (sc, hc, ks, s):
        h.free()
    return got


def _same(got, exp, what=""):
    for f in FIELDS:
        assert got[f].dtype == exp[f].dtype and got[f].tolist() == exp[f].tolist(), (what, f)
    assert got["bic"].view(np.uint64).tolist() == exp["bic"].view(np.uint64).tolist(), (what, "bic")


@pytest.mark.parametrize("k", [21, 32])
def test_crafted_cases(ctx, tmp_path, k):
    for name, (case, params, want) in Cs.crafted(k).items():
        exp = Cs.restate(case, params)
        assert want <= exp["trace"], name
        got = _run(ctx, case, tmp_path, name, params)
        _same(got, exp, name)
        assert got["host_kmers"] == 0 and got["count"] == len(exp["sizes"]) and got["new"] == len(exp["new_keys"])
    exp = Cs.restate(Cs.chain_case(k))
    assert len(exp["new_keys"]) == 1 and exp["good"][-1] == 0  # the new k-mer ends bad


@pytest.mark.parametrize("k", [10, 11, 21, 22, 32])
def test_key_and_quality_word_boundaries(ctx, tmp_path, k):
    case = Cs.random_case(k, 500 + k, 300, 12)
    sizes = case["sizes"].tolist()
    assert len(sizes) == 300 and min(sizes) == 1 and max(sizes) == 12
    assert case["qual_words"].shape[1] == {10: 1, 11: 2, 21: 2, 22: 3, 32: 3}[k]
    exp = Cs.restate(case)
    assert exp["stats"][1] > 0 and exp["stats"][4] > 0 and exp["good"].any() and not exp["good"].all()
    _same(_run(ctx, case, tmp_path, "rnd"), exp)


HOST_CHILD = """
import sys
import numpy as np
import spades_for_blackbird_amd as B
sys.path.insert(0, sys.argv[3])
from tests.test_gpu_subcluster import _load
ctx = B.Context(0)
s, ks, hc = _load(ctx, sys.argv[1], int(sys.argv[2]))
sc = hc.subcluster(ks)
r = sc.export()
np.savez(sys.argv[1] + ".host.npz", host_kmers=sc.host_kmers, **r)
"""


def test_size_classes_and_the_host_path(ctx, tmp_path):
    """64 | 65: wavefront and workgroup kernel; 256 | 257: workgroup kernel and host path"""
    k = 21
    case = Cs.sized_case(k, 5)
    assert sorted(case["sizes"].tolist()) == [64, 65, 256, 257]
    exp = Cs.restate(case)
    assert "maxcls_stop" in exp["trace"]
    got = _run(ctx, case, tmp_path, "sized")
    _same(got, exp)
    assert got["host_kmers"] == 257
    env = dict(os.environ, BBK_SUBCLUSTER_HOST="1")
    r = subprocess.run([sys.executable, "-c", HOST_CHILD, str(tmp_path / "sized"), str(k), ROOT], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    host = np.load(str(tmp_path / "sized") + ".host.npz")
    assert int(host["host_kmers"]) == 64 + 65 + 256 + 257
    for f in FIELDS + ("bic",):
        assert host[f].tobytes() == got[f].tobytes(), f


def test_cluster_order_of_the_file_does_not_matter(ctx, tmp_path):
    k = 21
    cases = [Cs.random_case(k, 900, 60, 12), Cs.chain_case(k)]
    # two new k-mers in different clusters: a chain next to a random case would collide, so the chain is built twice
    rng = np.random.default_rng(3)
    a, b = Cs.chain_case(21), Cs.chain_case(21)
    shift = Cs.sub(Cs.sub(0, 4, 1), 9, 2) ^ Cs.sub(0, 15, 3)
    items = []
    for case, x in ((a, 0), (b, shift)):
        for i, key in enumerate(case["keys"]):
            items.append((key ^ x, int(case["count"][i]), case["tq"][i], case["quals"][i]))
    two = Cs.make_case(k, items, [list(range(5)), list(range(5, 10))])
    for case in cases + [two]:
        exp = Cs.restate(case)
        order = rng.permutation(len(case["sizes"]))
        got = _run(ctx, case, tmp_path, "perm", cluster_order=order)
        _same(got, exp)
    assert len(exp["new_keys"]) == 2 and exp["members"][0] == 10 and exp["members"][6] == 11  # numbered by label


def _genome_reads(k, seed, n_reads=200):
    """(seq, qual) records drawn from both strands of a 300-base genome, 30-60 bases each, with substitutions so that
    Hamming clusters form; qualities uniform in [2, 41]"""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), 300))
    reads = []
    for i in range(n_reads):
        n = int(rng.integers(30, 61))
        st = int(rng.integers(0, 300 - n + 1))
        s = list(genome[st:st + n])
        if i % 3 == 0:
            j = int(rng.integers(0, n))
            s[j] = "ACGT"[("ACGT".index(s[j]) + int(rng.integers(1, 4))) % 4]
        s = "".join(s)
        if rng.random() < 0.5:
            s = KR.revcomp(s)
        reads.append((s, [int(x) for x in rng.integers(2, 42, len(s))]))
    return reads


def _upload(ctx, stretches):
    reads = ctx.reads_from_ascii([s for s, _ in stretches])
    offs = np.zeros(len(stretches) + 1, dtype=np.uint64)
    if stretches:
        offs[1:] = np.cumsum([len(q) for _, q in stretches], dtype=np.uint64)
    qb = np.array([x for _, q in stretches for x in q], dtype=np.uint8)
    return reads, ctx.quals(reads, qb, offs)


def _stretches(reads, k):
    out = []
    for seq, qual in reads:
        for s, n in KR.coalesce(KR.valid_starts(seq, qual, k), k):
            out.append((seq[s:s + n], qual[s:s + n]))
    return out


def _pipeline(ctx, reads, k):
    rd, qu = _upload(ctx, _stretches(reads, k))
    s = ctx.count(rd, k, B.BOTH_STRANDS)
    ks = s.kmer_stats()
    ks.push(rd, qu)
    ks.finish()
    hc = s.hamming_clusters()
    return s, ks, hc


def _restate_handles(s, ks, hc, k, params=None):
    cnt, tq, qw = ks.export()
    keys = [int(x) for x in s.export()[:, 0]] if len(s) else []
    return R.process(keys, k, cnt, tq, qw, hc.members(), hc.sizes(), params)


@pytest.mark.parametrize("k", [21, 32])
def test_end_to_end(ctx, k):
    reads = _genome_reads(k, 8100 + k)
    s, ks, hc = _pipeline(ctx, reads, k)
    sizes = hc.sizes()
    assert (sizes == 1).any() and (sizes > 1).any()
    sc = hc.subcluster(ks)
    exp = _restate_handles(s, ks, hc, k)
    _same(sc.export(), exp)
    assert sc.stats == dict(zip(sc.STATS, exp["stats"].tolist())) and exp["stats"][7] > 0


def test_empty_set(ctx):
    rd, qu = _upload(ctx, [("ACGTACGT", [30] * 8)])  # shorter than k: no k-mer
    s = ctx.count(rd, 21, B.BOTH_STRANDS)
    assert len(s) == 0
    ks = s.kmer_stats()
    ks.finish()
    sc = s.hamming_clusters().subcluster(ks)
    r = sc.export()
    assert len(sc) == 0 and sc.size == 0 and sc.new_kmers == 0 and sc.host_kmers == 0
    assert all(len(r[f]) == 0 for f in ("good", "members", "sizes", "per_cluster", "new_keys", "bic"))
    assert not r["errs"].any() and not r["stats"].any()


def test_refusals(ctx, tmp_path):
    L = B.load_library()
    k = 21
    case, other = Cs.random_case(k, 1, 10, 6), Cs.random_case(k, 2, 14, 6)
    _write_case(case, str(tmp_path / "a"))
    _write_case(other, str(tmp_path / "b"))
    s, ks, hc = _load(ctx, str(tmp_path / "a"), k)
    s2, ks2, hc2 = _load(ctx, str(tmp_path / "b"), k)
    assert len(s) != len(s2)

    def refused(fn, match):
        with pytest.raises(B.BBKError, match=match) as e:
            fn()
        assert "bbk error %d:" % ERR_ARG in str(e.value) and L.bbk_last_error()

    refused(lambda: hc2.subcluster(ks), "the set has")  # clusters of another size
    ks2._set = s
    refused(lambda: hc.subcluster(ks2), "another k-mer set")  # statistics of another set
    ks2._set = s2
    refused(lambda: hc.subcluster(ks, singleton_threshold=1.5), "outside \\[0, 1\\]")
    refused(lambda: hc.subcluster(ks, correct_threshold=-0.1), "outside \\[0, 1\\]")
    # unfinished statistics: counted ones, before finish
    rd, qu = _upload(ctx, _stretches(_genome_reads(k, 5, 20), k))
    s3 = ctx.count(rd, k, B.BOTH_STRANDS)
    ks3 = s3.kmer_stats()
    ks3.push(rd, qu)
    h3 = s3.hamming_clusters()
    refused(lambda: h3.subcluster(ks3), "bbk_kmerstats_finish")
    # loaded statistics take no more reads
    refused(lambda: ks.push(rd, qu), "read from a file")
    # files that do not fit
    n = len(case["keys"])
    mem = np.fromfile(str(tmp_path / "a.hamming"), dtype=np.uint64)
    bad = mem.copy()
    bad[1] = bad[0]
    bad.tofile(str(tmp_path / "dup.hamming"))
    shutil.copy(str(tmp_path / "a.hamming.idx"), str(tmp_path / "dup.hamming.idx"))
    refused(lambda: ctx.hamclusters_load(n, str(tmp_path / "dup.hamming")), "not a permutation")
    bad = mem.copy()
    bad[2] = n
    bad.tofile(str(tmp_path / "range.hamming"))
    shutil.copy(str(tmp_path / "a.hamming.idx"), str(tmp_path / "range.hamming.idx"))
    refused(lambda: ctx.hamclusters_load(n, str(tmp_path / "range.hamming")), "not a permutation")
    refused(lambda: ctx.hamclusters_load(n + 1, str(tmp_path / "a.hamming")), "lists %d members" % n)
    idx = np.fromfile(str(tmp_path / "a.hamming.idx"), dtype=np.uint64)
    mem.tofile(str(tmp_path / "sum.hamming"))
    idx[:-1].tofile(str(tmp_path / "sum.hamming.idx"))
    refused(lambda: ctx.hamclusters_load(n, str(tmp_path / "sum.hamming")), "sum to")
    refused(lambda: ctx.kmerstats_load(s2, str(tmp_path / "a.kmstat")), "does not hold")
    # no handle was left behind: a refused call leaves its output NULL
    import ctypes as C
    h = C.c_void_p()
    assert L.bbk_hamclusters_load(ctx._h, n, str(tmp_path / "dup.hamming").encode(), C.byref(h)) == ERR_ARG and not h.value
    p = B.engine.SubclusterParams(1.5, 0.9, 0.98, 1)
    assert L.bbk_hamclusters_subcluster(ctx._h, s._h, hc._h, ks._h, C.byref(p), C.byref(h)) == ERR_ARG and not h.value
    assert b"1.5" in L.bbk_last_error()


def test_kmstat_writer_across_a_block_boundary(ctx, tmp_path):
    """KmerStats.write and SubClusters.write share one writer that goes 2^20 records at a time: 2^20 + 3 k-mers, all of
    them singleton clusters, so the good bit of a record is the decision on its own total_qual"""
    import torch
    k, block = 21, 1 << 20
    n = block + 3
    keys = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)  # distinct, ascending, below 4^21
    rec = np.zeros(n, dtype=np.dtype([("c", "<u4"), ("tq", "<f4"), ("w", "<u8", (2,))]))
    count = (np.arange(1, n + 1, dtype=np.uint64) % 1000 + 1).astype(np.uint32)
    rec["c"] = count << 1
    rec["tq"] = np.where(np.arange(n) % 2 == 0, np.float32(0.015), np.float32(0.025))  # 1 - tq either side of 0.98
    rec["w"][:, 0] = keys * np.uint64(0x9E3779B97F4A7C15)
    rec["w"][:, 1] = (keys * np.uint64(0xBF58476D1CE4E5B9)) >> np.uint64(2)  # 6 * 21 = 126 bits: the top two stay clear
    prefix = str(tmp_path / "big")
    rec.tofile(prefix + ".kmstat")
    np.arange(n, dtype=np.uint64).tofile(prefix + ".hamming")
    np.ones(n, dtype=np.uint64).tofile(prefix + ".hamming.idx")
    d = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    s = ctx.kmerset_from_device(d, n, k)
    ks, hc = ctx.kmerstats_load(s, prefix + ".kmstat"), ctx.hamclusters_load(n, prefix + ".hamming")
    sc = hc.subcluster(ks)
    assert len(sc) == n and sc.new_kmers == 0 and sc.host_kmers == 0
    ks.write(prefix + ".again.kmstat")
    sc.write(prefix + ".sc")
    for h in (sc, hc, ks, s):
        h.free()
    edge = range(block - 2, block + 3)  # the records either side of the boundary by name, then everything
    again = np.fromfile(prefix + ".again.kmstat", dtype=rec.dtype)
    assert len(again) == n
    for i in edge:
        assert again[i].tobytes() == rec[i].tobytes(), i
    assert open(prefix + ".again.kmstat", "rb").read() == rec.tobytes()
    good = (np.float32(1) - rec["tq"]).astype(np.float64) > 0.98  # sc_good_quality: a float subtraction, then widened
    assert good[0] and not good[1]
    exp = rec.copy()
    exp["c"] |= good.astype(np.uint32)
    got = np.fromfile(prefix + ".sc.kmstat", dtype=rec.dtype)
    assert len(got) == n
    for i in edge:
        assert got[i].tobytes() == exp[i].tobytes(), i
    assert open(prefix + ".sc.kmstat", "rb").read() == exp.tobytes()
    m = 1000
    restated = R.process(keys[:m], k, count[:m], rec["tq"][:m], rec["w"][:m], np.arange(m), np.ones(m, dtype=np.uint64))
    assert (got["c"][:m] & 1).astype(np.uint8).tolist() == restated["good"].tolist()
    assert open(prefix + ".sc.subclusters", "rb").read() == np.arange(n, dtype=np.uint64).tobytes()


# md5 of the files `spades-kmerdata -k 21 -o out --cluster -b 60000 tests/golden/ecoli_1K_1.fq.gz` writes, from the binary
# and library of the commit before --subcluster existed
PARENT_MD5 = {
    ".kmers": "aee18ac251b62d76ce90421d0d000821",
    ".kmstat": "276626849d59fc585186186b0fb9b035",
    ".hamming": "111033ea70613750ce7ba8608a6352c1",
    ".hamming.idx": "5937348968b3f61bbddef4c447cc5fd0",
}


def _md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def test_cli(ctx, tmp_path, golden_dir):
    k = 21
    exe = [e for e in build_host.build() if e.endswith("spades-kmerdata")][0]
    path = os.path.join(golden_dir, "ecoli_1K_1.fq.gz")
    plain, prefix = str(tmp_path / "plain"), str(tmp_path / "out")
    r = subprocess.run([exe, "-k", str(k), "-o", plain, "--cluster", "-b", "60000", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Subclustering" not in r.stdout + r.stderr
    assert sorted(os.listdir(str(tmp_path))) == sorted("plain" + e for e in PARENT_MD5)
    assert {e: _md5(plain + e) for e in PARENT_MD5} == PARENT_MD5
    r = subprocess.run([exe, "-k", str(k), "-o", prefix, "--subcluster", "-b", "60000", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    log = r.stdout + r.stderr
    for e in (".kmers", ".hamming", ".hamming.idx"):
        assert _md5(prefix + e) == PARENT_MD5[e]
    # the same run from Python
    with gzip.open(path, "rt") as f:
        lines = f.read().split("\n")
    reads = [(lines[i + 1], [ord(c) - 33 for c in lines[i + 3]]) for i in range(0, len(lines) - 3, 4)]
    s, ks, hc = _pipeline(ctx, reads, k)
    sc = hc.subcluster(ks)
    exp = sc.export()
    n = len(s)
    rec = np.fromfile(prefix + ".kmstat", dtype=np.dtype([("c", "<u4"), ("tq", "<f4"), ("w", "<u8", (2,))]))
    assert len(rec) == n + sc.new_kmers
    assert (rec["c"] & 1).astype(np.uint8).tolist() == exp["good"].tolist() and exp["good"].any()
    parent = np.fromfile(plain + ".kmstat", dtype=rec.dtype)
    assert (rec["c"][:n] >> 1).tolist() == (parent["c"] >> 1).tolist() and rec[:n]["tq"].tobytes() == parent["tq"].tobytes()
    assert rec[:n]["w"].tobytes() == parent["w"].tobytes()
    assert not rec["c"][n:].any() and (rec["tq"][n:] == 1).all() and not rec["w"][n:].any()
    assert open(prefix + ".subclusters", "rb").read() == exp["members"].tobytes()
    assert open(prefix + ".subclusters.idx", "rb").read() == exp["sizes"].tobytes()
    assert open(prefix + ".newkmers", "rb").read() == exp["new_keys"].tobytes()
    sc.write(str(tmp_path / "py"))
    for e in (".kmstat", ".subclusters", ".subclusters.idx", ".newkmers"):
        assert _md5(str(tmp_path / "py") + e) == _md5(prefix + e), e
    st = sc.stats
    assert "Total %d non-read kmers were generated" % st["newkmers"] in log
    assert "Total singleton hamming clusters: %d. Among them %d (" % (st["tsingl"], st["gsingl"]) in log
    assert "Total singleton subclusters: %d. Among them %d (" % (st["tcsingl"], st["gcsingl"]) in log
    assert "Total non-singleton subcluster centers: %d. Among them %d (" % (st["tcls"], st["gcls"]) in log
    assert "Total solid k-mers: %d" % (st["gsingl"] + st["gcsingl"] + st["gcls"]) in log
    assert st["tsingl"] > 0 and st["tncls"] > 0
    # a threshold outside [0, 1] is refused by the library
    r = subprocess.run([exe, "-k", str(k), "-o", prefix + "2", "--subcluster", "--singleton-threshold", "1.5", path],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "outside [0, 1]" in r.stdout + r.stderr
