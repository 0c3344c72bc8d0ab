"""GPU: BayesHammer's per-k-mer statistics (bbk_kmerstats_*, csrc/kmerstat.hip) and spades-kmerdata against the
restatement (tests/kmerdata_restated.py).  Counts and quality words are compared exactly; total_qual by the derived
bound |device - P| <= (n + 1) * 2^-22 * P + n * 2^-149 around the exact product P of the restatement's float32 factors
(kmerdata_restated.total_qual_bound), whose condition -- every pushed window has 1 - cp >= 2^-10, reads of at most 1024
bases -- the inputs keep and the first test asserts."""
import ctypes as C
import gzip
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build_host
from tests import kmerdata_restated as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [10, 11, 21, 22, 32]  # QualBitSet words 1 -> 2 -> 3; sums 10 and 21 straddle the two word boundaries


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def _stretches(reads, k):
    """the engine reads of (seq, qual) records: one per run of consecutive valid starts"""
    out = []
    for seq, qual in reads:
        for s, n in R.coalesce(R.valid_starts(seq, qual, k), k):
            out.append((seq[s:s + n], qual[s:s + n]))
    return out


def _upload(ctx, stretches):
    reads = ctx.reads_from_ascii([s for s, _ in stretches])
    offs = np.zeros(len(stretches) + 1, dtype=np.uint64)
    if stretches:
        offs[1:] = np.cumsum([len(q) for _, q in stretches], dtype=np.uint64)
    qb = np.array([x for _, q in stretches for x in q], dtype=np.uint8)
    return reads, ctx.quals(reads, qb, offs)


def _push(ctx, ks, stretches):
    reads, quals = _upload(ctx, stretches)
    ks.push(reads, quals)
    quals.free()
    reads.free()


def _check(keys, k, got, expected):
    """got = KmerStats.export(); expected = {k-mer: (count, [sums], [float32 factors])} for exactly the k-mers of keys"""
    cnt, tq, qw = got
    by_key = {R.kmer_key(km): v for km, v in expected.items()}
    assert sorted(by_key) == keys, "the restatement's k-mers are not the set"
    assert qw.shape == (len(keys), (6 * k + 63) // 64)
    worst = Fraction(0)
    for i, key in enumerate(keys):
        c, sums, factors = by_key[key]
        assert int(cnt[i]) == c, (i, key)
        assert [int(x) for x in qw[i]] == R.pack_le(sums), (i, key)
        p, bound = R.total_qual_bound(factors)
        err = abs(Fraction(float(tq[i])) - p)
        assert err <= bound, (i, key, float(tq[i]), float(p), float(err / bound))
        worst = max(worst, err / bound)
    print("k = %d: %d k-mers, worst total_qual error %.3f of the bound" % (k, len(keys), float(worst)))


def _as_tuples(data):
    return {km: (st.count, st.qual.values(), st.factors) for km, st in data.items()}


def _keys(s):
    return [int(x) for x in s.export()[:, 0]]


def _genome_reads(k, seed, n_reads=200, palindrome=False):
    """(seq, qual) records drawn from both strands of a 300-base genome, 30-60 bases each, qualities uniform in
    [2, 41], some with interior Ns and bad ends, plus the crafted corner reads"""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), 300))
    pal = None
    if palindrome:
        half = "".join(rng.choice(list("ACGT"), k // 2))
        pal = half + R.revcomp(half)
        genome = genome[:100] + pal + genome[100 + k:]
    reads = []
    for i in range(n_reads):
        n = int(rng.integers(30, 61))
        st = int(rng.integers(0, 300 - n + 1))
        if palindrome and i < 6:  # reads that cover the planted k-mer, untrimmed
            st, n = 95 - i, k + 12
        s = genome[st:st + n]
        if rng.random() < 0.5:
            s = R.revcomp(s)
        q = [int(x) for x in rng.integers(2, 42, len(s))]
        if palindrome and i < 6:
            q = [int(x) for x in rng.integers(20, 42, len(s))]
        elif i % 7 == 0:  # interior Ns
            for j in rng.integers(5, len(s) - 5, 2):
                s = s[:j] + "N" + s[j + 1:]
        elif i % 7 == 1:  # q < 2 ends
            q[:2] = [0, 1]
            q[-3:] = [1, 1, 0]
        elif i % 7 == 2:  # q <= 4 ends
            q[:3] = [4, 3, 2]
            q[-2:] = [3, 4]
        reads.append((s, q))
    reads += [(s, q) for _, s, q in R.crafted_reads(k, rng)]
    return reads, pal


@pytest.mark.parametrize("k", KS)
def test_against_the_restatement(ctx, k):
    pal_k = k in (10, 22, 32)
    reads, pal = _genome_reads(k, 7000 + k, palindrome=pal_k)
    assert all(len(s) <= 1024 for s, _ in reads) and R.min_window_complement(reads, k) >= 2 ** -10
    kinds = [len(R.valid_starts(s, q, k)) for s, q in reads]
    assert 0 in kinds and 1 in kinds
    st = _stretches(reads, k)
    assert any(len(s) == k for s, _ in st)
    rd, qu = _upload(ctx, st)
    s = ctx.count(rd, k, B.BOTH_STRANDS)
    keys = _keys(s)
    ks = s.kmer_stats()
    assert len(ks) == len(keys)
    ks.push(rd, qu)
    ks.finish()
    exp = _as_tuples(R.fill_kmer_data(reads, k))
    got = ks.export()
    _check(keys, k, got, exp)
    assert int(got[0].max()) > 3 and int(ks.qual_matrix().max()) == 63  # counts exceed 1, sums saturate
    assert ks.qual_matrix().tolist() == [exp_v[1] for _, exp_v in sorted((R.kmer_key(km), v) for km, v in exp.items())]
    if pal_k:
        i = keys.index(R.kmer_key(pal))
        assert R.revcomp(pal) == pal and got[0][i] >= 2 and got[0][i] % 2 == 0
    ks.free()
    s.free()


def test_masking(ctx):
    """a quality of 70 enters the sums as 6, 64 as 0, 93 as 29 -- and the probabilities see the whole value"""
    k = 21
    rng = np.random.default_rng(31)
    genome = "".join(rng.choice(list("ACGT"), 200))
    pattern = [70, 93, 64, 30, 12, 41, 63]
    reads = []
    for st in rng.integers(0, 150, 60):
        s = genome[st:st + 50]
        s = R.revcomp(s) if rng.random() < 0.5 else s
        reads.append((s, [pattern[i % 7] for i in range(len(s))]))
    assert R.min_window_complement(reads, k) >= 2 ** -10
    st = _stretches(reads, k)
    assert [s for s, _ in st] == [s for s, _ in reads]  # nothing is trimmed
    rd, qu = _upload(ctx, st)
    s = ctx.count(rd, k, B.BOTH_STRANDS)
    ks = s.kmer_stats()
    ks.push(rd, qu)
    ks.finish()
    exp = _as_tuples(R.fill_kmer_data(reads, k))
    _check(_keys(s), k, ks.export(), exp)
    singles = [v for v in exp.values() if v[0] == 1]
    assert singles and all(set(v[1]) <= {6, 29, 0, 30, 12, 41, 63} for v in singles)


def test_underflow(ctx):
    k = 21
    rng = np.random.default_rng(77)
    kmers = ["".join(rng.choice(list("ACGT"), k)) for _ in range(5)]
    copies = [600, 14, 15, 16, 17]
    reads = [(km, [40] * k) for km, n in zip(kmers, copies) for _ in range(n)]
    st = _stretches(reads, k)
    assert len(st) == sum(copies)
    rd, qu = _upload(ctx, st)
    s = ctx.count(rd, k, B.BOTH_STRANDS)
    keys = _keys(s)
    assert len(keys) == 10
    ks = s.kmer_stats()
    ks.push(rd, qu)
    ks.finish()
    got = ks.export()
    _check(keys, k, got, R.fill_kmer_data_fast(reads, k))
    for km in (kmers[0], R.revcomp(kmers[0])):
        i = keys.index(R.kmer_key(km))
        assert got[0][i] == 600 and got[1][i] == 0.0 and [int(x) for x in got[2][i]] == R.pack_le([63] * k)
    tiny = np.finfo(np.float32).tiny
    in_range = [float(got[1][keys.index(R.kmer_key(km))]) for km in kmers[1:]]
    assert in_range[0] > 0 and all(x < 4 * tiny for x in in_range) and in_range == sorted(in_range, reverse=True)


def test_same_bytes_for_any_batching_and_order(ctx):
    k = 21
    reads, _ = _genome_reads(k, 7000 + k)
    st = _stretches(reads, k)
    rd, qu = _upload(ctx, st)
    s = ctx.count(rd, k, B.BOTH_STRANDS)
    results = []
    for batches in ([st], [st[0::3], st[1::3], st[2::3]], [st[2::3][::-1], st[0::3][::-1], st[1::3][::-1]]):
        ks = s.kmer_stats()
        for b in batches:
            _push(ctx, ks, b)
        ks.finish()
        results.append(b"".join(a.tobytes() for a in ks.export()))
        ks.free()
    assert results[0] == results[1] == results[2]
    assert len(results[0]) == len(s) * (4 + 4 + 16)


def test_kmers_outside_the_set_are_skipped(ctx):
    k = 21
    reads, _ = _genome_reads(k, 7100)
    half = reads[:len(reads) // 2]
    rd, qu = _upload(ctx, _stretches(half, k))
    s = ctx.count(rd, k, B.BOTH_STRANDS)
    keys = _keys(s)
    in_set = set(R.fill_kmer_data_fast(half, k))
    everything = R.fill_kmer_data_fast(reads, k)
    assert len(in_set) < len(everything)
    exp = _as_tuples(R.fill_kmer_data(reads, k, kmer_set=in_set))
    assert any(exp[km][0] > R.fill_kmer_data_fast(half, k)[km][0] for km in in_set)  # occurrences from both halves
    ks = s.kmer_stats()
    _push(ctx, ks, _stretches(reads, k))
    ks.finish()
    _check(keys, k, ks.export(), exp)


def test_refusals(ctx, tmp_path):
    reads, _ = _genome_reads(21, 7200, n_reads=20)
    st = _stretches(reads, 21)
    rd, qu = _upload(ctx, st)
    with pytest.raises(B.BBKError, match="canonical only"):
        ctx.count(rd, 21, B.CANONICAL).kmer_stats()
    with pytest.raises(B.BBKError, match="final_kmers order"):
        ctx.count(rd, 21, B.BOTH_STRANDS | B.REFERENCE_ORDER).kmer_stats()
    long_reads = ctx.reads_from_ascii(["ACGT" * 12])
    with pytest.raises(B.BBKError, match="k = 33"):
        ctx.count(long_reads, 33, B.BOTH_STRANDS).kmer_stats()
    # a quality string of another length, another number of quality strings, a quality above 93
    offs = np.cumsum([0] + [len(q) for _, q in st]).astype(np.uint64)
    qb = np.array([x for _, q in st for x in q], dtype=np.uint8)
    bad = offs.copy()
    bad[1:] += 1
    with pytest.raises(B.BBKError, match="bases and"):
        ctx.quals(rd, np.append(qb, 0).astype(np.uint8), bad)
    with pytest.raises(B.BBKError, match="quality strings for"):
        ctx.quals(rd, qb, offs[:-1])
    high = qb.copy()
    high[3] = 94
    with pytest.raises(B.BBKError, match="quality 94"):
        ctx.quals(rd, high, offs)
    # qualities of other reads; export before finish
    s = ctx.count(rd, 21, B.BOTH_STRANDS)
    ks = s.kmer_stats()
    rd2, qu2 = _upload(ctx, st)
    with pytest.raises(B.BBKError, match="not made for these reads"):
        ks.push(rd, qu2)
    ks.push(rd, qu)
    with pytest.raises(B.BBKError, match="bbk_kmerstats_finish"):
        ks.export()
    ks.finish()
    ks.write(str(tmp_path / "ok.kmstat"))
    assert os.path.getsize(str(tmp_path / "ok.kmstat")) == 24 * len(s)
    # a count of 2^31 cannot be written as count << 1: made through the test-only entry point, not by counting
    L = B.load_library()
    L.bbk_kmerstats_test_add_count.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32]
    before = int(ks.export()[0][5])
    assert L.bbk_kmerstats_test_add_count(ks._h, 5, 2 ** 31 - before - 1) == 0
    ks.finish()
    assert int(ks.export()[0][5]) == 2 ** 31 - 1
    ks.write(str(tmp_path / "max.kmstat"))
    assert L.bbk_kmerstats_test_add_count(ks._h, 5, 1) == 0
    ks.finish()
    assert int(ks.export()[0][5]) == 2 ** 31
    with pytest.raises(B.BBKError, match="2\\^31 occurrences"):
        ks.write(str(tmp_path / "over.kmstat"))


def test_cli(ctx, tmp_path, golden_dir):
    k = 21
    exe = [e for e in build_host.build() if e.endswith("spades-kmerdata")][0]
    path = os.path.join(golden_dir, "ecoli_1K_1.fq.gz")
    prefix = str(tmp_path / "out")
    r = subprocess.run([exe, "-k", str(k), "-o", prefix, "--cluster", "-b", "60000", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with gzip.open(path, "rt") as f:
        lines = f.read().split("\n")
    reads = [(lines[i + 1], [ord(c) - 33 for c in lines[i + 3]]) for i in range(0, len(lines) - 3, 4)]
    assert len(reads) == 2054 and R.min_window_complement(reads[:200], k) >= 2 ** -10
    # the set: the same stretches pushed through Python, written as spades-hamcluster writes <prefix>.kmers
    rd, qu = _upload(ctx, _stretches(reads, k))
    s = ctx.count(rd, k, B.BOTH_STRANDS)
    assert open(prefix + ".kmers", "rb").read() == s.export().tobytes()
    keys = _keys(s)
    rec = np.fromfile(prefix + ".kmstat", dtype=np.dtype([("c", "<u4"), ("tq", "<f4"), ("w", "<u8", (2,))]))
    assert rec.itemsize == 24 and len(rec) == len(keys)
    assert not (rec["c"] & 1).any()  # the good bit
    _check(keys, k, (rec["c"] >> 1, rec["tq"], rec["w"]), R.fill_kmer_data_fast(reads, k))
    # the same statistics through Python, byte for byte
    ks = s.kmer_stats()
    ks.push(rd, qu)
    ks.finish()
    ks.write(str(tmp_path / "py.kmstat"))
    assert open(prefix + ".kmstat", "rb").read() == open(str(tmp_path / "py.kmstat"), "rb").read()
    h = s.hamming_clusters()
    assert open(prefix + ".hamming", "rb").read() == h.members().tobytes()
    assert open(prefix + ".hamming.idx", "rb").read() == h.sizes().tobytes()
    # FASTA has no qualities
    fa = tmp_path / "a.fa"
    fa.write_text(">x\n" + "ACGT" * 10 + "\n")
    r = subprocess.run([exe, "-k", str(k), "-o", prefix + "2", str(fa)], capture_output=True, text=True)
    assert r.returncode != 0 and "FASTQ" in r.stderr
