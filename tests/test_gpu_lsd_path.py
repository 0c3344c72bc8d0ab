"""GPU: the general (LSD) path of counting, merging and the extension index, and the sort / unique / scan primitives it
is built on (count.hip: LsdSort behind dedup_reads' extract + sort + unique, lsd_sort_unique, expand_both_strands'
expand + sort and the ascending export of a final_kmers set; sort.hip / unique.hip / scan.hip: sort_records, unique_records,
exclusive_scan_u64).

The engine takes this path whenever an MSD pass declines (one k-mer making up more than a quarter of a batch: poly-A
or amplicon libraries), and finishes oversized MSD buckets with the same primitives.  BBK_DISABLE_MSD=1 forces it (read
on every call, so monkeypatch is enough).  Every case checks through the kernel-family launch counts of the profiler
(or the BBK_VERBOSE lines) that the intended path ran, and compares with the CPU oracle or a numpy reduce.

Count overflow has one rule on every path: u32 multiplicities wrap modulo 2^32, as the reference's uint32_t += does
(common/stages/construction.cpp:29, coverage_hash_map_builder.hpp:34-35)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from oracle import oracle as O
from spades_for_blackbird_amd.tools import gfa_canon
from tests.helpers import rc, synth_reads
from tests.test_gpu_count import check_ref_order_by_extra_pass

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LSD_FAMILIES = ("extract", "expand", "hist", "scatter", "unique")
MSD_FAMILIES = ("k_part_reads_narrow", "k_part_reads", "k_bucket_hash", "k_bucket_hashidx", "k_bucket_dist", "k_bucket",
                "k_sk_dedup", "k_sk_dedup_B", "k_sk_part1")
BUCKET_FAMILIES = ("k_bucket_hash", "k_bucket_hashidx", "k_bucket_dist", "k_bucket")
TILE = {1: 4096, 2: 2048, 3: 2048, 4: 1024}  # SortCfg<W>::TILE (sort.hip)
K_CHUNK = 256                                # tiles per chunk of k_colsum / k_tile_offsets
UNIQ_TILE = 2048                             # kUniqTile of k_head_count / k_head_compact
SCAN_TILE = 2048                             # kScanTile of exclusive_scan_u64
WRAP = 1 << 32


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = B.Context(0, stream=torch.cuda.current_stream())
    yield c
    c.close()


@pytest.fixture
def lsd(ctx, monkeypatch):
    """the forced general path, profiler on and empty"""
    monkeypatch.setenv("BBK_DISABLE_MSD", "1")
    ctx.profile(True)
    ctx.profile_reset()
    yield ctx
    ctx.profile(False)
    ctx.profile_reset()


def launches(ctx, fam):
    return ctx.profile_get(fam)["launches"]


def assert_lsd(ctx, *families):
    """the calls since the last check launched every one of `families` and no MSD / super-k-mer kernel"""
    for f in families:
        assert f in LSD_FAMILIES
        assert launches(ctx, f) > 0, "no %s launch: the general path did not run" % f
    ran = {f: launches(ctx, f) for f in MSD_FAMILIES}
    assert not any(ran.values()), "MSD kernels ran on the forced general path: %r" % ran
    ctx.profile_reset()


def assert_path(ctx, forced):
    """forced: the general path alone ran; otherwise the MSD bucket kernels ran (unless the environment disables them)"""
    if forced:
        assert_lsd(ctx, "hist", "scatter", "unique")
    elif not os.environ.get("BBK_DISABLE_MSD"):
        assert sum(launches(ctx, f) for f in BUCKET_FAMILIES) > 0, "the MSD path did not run"
    ctx.profile_reset()


def msd_run(ctx, monkeypatch, fn):
    """fn() with the MSD path allowed again (as far as the environment allows it), profiler counts discarded"""
    with monkeypatch.context() as m:
        m.delenv("BBK_DISABLE_MSD", raising=False)
        out = fn()
    ctx.profile_reset()
    return out


def lex(keys):
    return np.lexsort(tuple(keys[:, w] for w in range(keys.shape[1] - 1, -1, -1)))


def expect_merge(keys, counts):
    """distinct keys ascending (word 0 most significant), counts summed modulo 2^32"""
    order = lex(keys)
    ks, cs = keys[order], counts[order].astype(np.uint64)
    head = np.ones(len(ks), dtype=bool)
    head[1:] = np.any(ks[1:] != ks[:-1], axis=1)
    starts = np.flatnonzero(head)
    sums = np.add.reduceat(cs, starts) if len(cs) else np.zeros(0, dtype=np.uint64)
    return ks[head], (sums % np.uint64(WRAP)).astype(np.uint32)


def to_device(keys, counts=None):
    import torch
    dk = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).cuda()
    dc = torch.from_numpy(np.ascontiguousarray(counts).view(np.int32)).cuda() if counts is not None else None
    torch.cuda.synchronize()
    return dk, dc


def from_device(ctx, keys, k, counts=None, flags=0):
    dk, dc = to_device(keys, counts)
    s = ctx.kmerset_from_device(dk, len(keys), k, d_counts=dc, flags=flags)
    return s, (dk, dc)


def used_bits_mask(k):
    """per word: the bits a k-mer uses (2 bits a base, the last word only its low 2k - 64(W-1) bits)"""
    nw = B.engine.words(k)
    m = np.full(nw, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    top = 2 * k - 64 * (nw - 1)
    if top < 64:
        m[nw - 1] = np.uint64((1 << top) - 1)
    return m


def random_keys(rng, n, k):
    nw = B.engine.words(k)
    return rng.integers(0, 2**64, size=(n, nw), dtype=np.uint64, endpoint=False) & used_bits_mask(k)


def read_mix(k):
    """test_gpu_count.test_vs_oracle_all_k's reads, plus reads holding k-1, k, 63, 64 and 65 k-mers: k_extract runs one
    wavefront per read with lanes striding by 64 positions"""
    reads = synth_reads(400, read_len=150, genome_len=3000, sub_rate=0.01, seed=k, n_rate=0.002)
    reads += ["", "A", "ACGT" * 40, "N" * 50, "acgtnACGTTGCA" * 12, "T" * 150]
    rng = np.random.default_rng(1000 + k)
    for L in (k - 1, k, k + 62, k + 63, k + 64):
        if L > 0:
            reads.append("".join("ACGT"[i] for i in rng.integers(0, 4, size=L)))
    return reads


def canonical_ref(reads, k):
    """canonical k-mers (min(kmer, rc) in base order) of the LongestValid runs, ascending, with their multiplicities"""
    fwd = {}
    for s in reads:
        a, b = O.longest_valid(s)
        seg = s[a:b].upper()
        for p in range(len(seg) - k + 1):
            x = seg[p:p + k]
            fwd[x] = fwd.get(x, 0) + 1
    canon = {}
    for x, c in fwd.items():
        y = rc(x)
        m = x if x <= y else y
        canon[m] = canon.get(m, 0) + c
    nw = B.engine.words(k)
    keys = np.array([O.kmer_words(m) for m in canon], dtype=np.uint64).reshape(-1, nw)
    cnt = np.array(list(canon.values()), dtype=np.uint32)
    order = lex(keys)
    return keys[order], cnt[order]


# ---- a. the forced general path against the oracle --------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 4, 5, 16, 21, 22, 31, 32, 33, 55, 63, 64, 65, 77, 96, 97, 127])
def test_forced_count_vs_oracle(lsd, monkeypatch, k):
    ctx = lsd
    reads = read_mix(k)
    r = ctx.reads_from_ascii(reads)
    exp, expc = O.kmercount(reads, k, 16, 2, with_counts=True)
    ck, cc = canonical_ref(reads, k)
    n_inst = int(cc.sum())

    # both strands + counts, exported in the final_kmers order (the XXH3 digit pass of export_ordered)
    s = ctx.count(r, k, B.BOTH_STRANDS | B.WITH_COUNTS)
    got, gotc = s.export(B.ORDER_REFERENCE_BUCKETS16, with_counts=True)
    assert_lsd(ctx, "extract", "expand", "hist", "scatter", "unique")
    assert np.array_equal(got, exp) and np.array_equal(gotc, expc)
    assert s.instances == 2 * n_inst

    # stored in the final_kmers order
    s = ctx.count(r, k, B.BOTH_STRANDS | B.REFERENCE_ORDER)
    assert s.device_keys()[1] == B.ORDER_REFERENCE_BUCKETS16
    assert np.array_equal(s.export(B.ORDER_REFERENCE_BUCKETS16), exp)
    assert_lsd(ctx, "extract", "expand", "hist", "scatter", "unique")

    # canonical + counts, ascending
    cs = ctx.count(r, k, B.CANONICAL | B.WITH_COUNTS)
    gk, gc = cs.export(B.ORDER_SORTED, with_counts=True)
    assert_lsd(ctx, "extract", "hist", "scatter", "unique")
    assert np.array_equal(gk, ck) and np.array_equal(gc, cc)
    assert cs.instances == n_inst

    # canonical, unsorted -> owner partition (the owner digit pass): per segment the MSD run's set
    def owners(flags):
        u = ctx.count(r, k, flags)
        keys = np.zeros((len(u), B.engine.words(k)), dtype=np.uint64)
        cnt = np.zeros(len(u), dtype=np.uint32)
        per = u.export_by_owner(4, keys, cnt)
        segs, o = [], 0
        for c in per.tolist():
            sk, sc = keys[o:o + c], cnt[o:o + c]
            order = lex(sk)
            segs.append((sk[order], sc[order]))
            o += c
        return segs
    flags = B.CANONICAL | B.UNSORTED | B.WITH_COUNTS
    lsd_segs = owners(flags)
    assert_lsd(ctx, "extract", "hist", "scatter", "unique")
    msd_segs = msd_run(ctx, monkeypatch, lambda: owners(flags))
    for (ak, ac), (bk, bc) in zip(lsd_segs, msd_segs):
        assert np.array_equal(ak, bk) and np.array_equal(ac, bc)
    allk = np.concatenate([sk for sk, _ in lsd_segs])
    allc = np.concatenate([sc for _, sc in lsd_segs])
    order = lex(allk)
    assert np.array_equal(allk[order], ck) and np.array_equal(allc[order], cc)

    # both strands of the canonical set: even k doubles the counts of self-reverse-complementary k-mers
    bs = cs.both_strands()
    got, gotc = bs.export(B.ORDER_REFERENCE_BUCKETS16, with_counts=True)
    assert_lsd(ctx, "expand", "hist", "scatter", "unique")
    assert np.array_equal(got, exp) and np.array_equal(gotc, expc)

    # streaming: 4 pushes + finish (lsd_sort_unique with SUM for the merge, sort_distinct for the order)
    cuts = [0, len(reads) // 4, len(reads) // 2, 3 * len(reads) // 4, len(reads)]
    for flags in (B.CANONICAL | B.WITH_COUNTS, B.CANONICAL, B.BOTH_STRANDS | B.WITH_COUNTS):
        c = ctx.counter(k, flags)
        for a, b in zip(cuts, cuts[1:]):
            c.push_ascii(reads[a:b])
        fs = c.finish()
        if flags & B.CANONICAL:
            assert_lsd(ctx, "extract", "hist", "scatter", "unique")
            if flags & B.WITH_COUNTS:
                gk, gc = fs.export(B.ORDER_SORTED, with_counts=True)
                assert np.array_equal(gk, ck) and np.array_equal(gc, cc)
            else:
                assert np.array_equal(fs.export(B.ORDER_SORTED), ck)
        else:
            assert_lsd(ctx, "extract", "expand", "hist", "scatter", "unique")
            got, gotc = fs.export(B.ORDER_REFERENCE_BUCKETS16, with_counts=True)
            assert np.array_equal(got, exp) and np.array_equal(gotc, expc)


def test_forced_wide_ref_order_by_extra_pass_with_payload(lsd, monkeypatch):
    """test_gpu_count's wide-key case on the forced general path: the ascending result of expand + sort + unique takes
    the one stable pass on the XXH3 bucket, counts alongside"""
    monkeypatch.setenv("BBK_NO_WIDE_REF", "1")
    check_ref_order_by_extra_pass(lsd, 77)
    assert_lsd(lsd, "extract", "expand", "hist", "scatter", "unique")


def oracle_ext(reads, k):
    x = O.ExtIndex(reads, k, 1)
    order = lex(x.kmers)
    return x.kmers[order], x.masks[order]


def mirror(masks):
    """InOutMask bit i -> bit 7 - i (the byte of the reverse-complement orientation)"""
    bits = np.unpackbits(masks[:, None], axis=1)
    return np.packbits(bits[:, ::-1], axis=1)[:, 0]


def palindromes(reads, k):
    """rows (as tuples) of the self-reverse-complementary k-mers of the reads (even k only)"""
    out = set()
    for s in reads:
        a, b = O.longest_valid(s)
        seg = s[a:b].upper()
        for p in range(len(seg) - k + 1):
            x = seg[p:p + k]
            if x == rc(x):
                out.add(tuple(O.kmer_words(x)))
    return out


def assert_masks(reads, k, gk, gm, ek, em):
    """Equal to the oracle, except for one known divergence at even k: a self-reverse-complementary k-mer gets the
    bit of the strand the read shows (bit c or its mirror 7 - c), the reference the bit of the canonical (k+1)-mer
    (FillExtensionsFromIndex, kmer_extension_index_builder.hpp:44-58).  Both paths do this the same way, and the graph
    builder refuses even k.  There the union of the two orientations must agree."""
    assert np.array_equal(gk, ek)
    pset = palindromes(reads, k) if k % 2 == 0 else set()
    pal = np.array([tuple(row) in pset for row in gk.tolist()], dtype=bool)
    assert np.array_equal(gm[~pal], em[~pal])
    assert np.array_equal(gm[pal] | mirror(gm[pal]), em[pal] | mirror(em[pal]))


@pytest.mark.parametrize("k", [3, 5, 21, 31, 32, 33, 63, 64, 65, 125])
def test_forced_extindex_vs_oracle(lsd, monkeypatch, k):
    """keys + InOutMask bytes (k_extract<W, 1>'s mask bits, reduced with OR by unique_records) against the oracle and,
    byte for byte, the MSD path; pushed batches equal one shot"""
    ctx = lsd
    reads = read_mix(k)
    ek, em = oracle_ext(reads, k)
    r = ctx.reads_from_ascii(reads)
    x = ctx.extindex(r, k)
    gk, gm = x.export()
    assert_lsd(ctx, "extract", "hist", "scatter", "unique")
    assert_masks(reads, k, gk, gm, ek, em)
    mk, mm = msd_run(ctx, monkeypatch, lambda: ctx.extindex(r, k).export())
    assert np.array_equal(gk, mk) and np.array_equal(gm, mm)
    b = ctx.extbuilder(k)
    third = len(reads) // 3
    for part in (reads[:third], reads[third:2 * third], reads[2 * third:]):
        b.push(ctx.reads_from_ascii(part))
    bk, bm = b.finish().export()
    assert_lsd(ctx, "extract", "hist", "scatter", "unique")
    assert np.array_equal(bk, gk) and np.array_equal(bm, gm)


@pytest.mark.parametrize("k", [21, 33])
def test_forced_gfa_vs_oracle(lsd, k, tmp_path):
    ctx = lsd
    reads = synth_reads(600, read_len=150, genome_len=5000, sub_rate=0.01, seed=300 + k, n_rate=0.001)
    x = ctx.extindex(ctx.reads_from_ascii(reads), k)
    assert_lsd(ctx, "extract", "hist", "scatter", "unique")
    u = ctx.unitigs(x)
    p = str(tmp_path / "g.gfa")
    u.write_gfa(p)
    with open(p) as f:
        txt = f.read()
    exp = O.ExtIndex(reads, k, 1).unitigs().gfa()[0]
    assert gfa_canon.canon_md5(txt, k) == gfa_canon.canon_md5(exp, k)


def test_forced_median_filter(lsd):
    """bbk_reads_median_filter on a canonical set counted by the general path (test_gpu_count's direct evaluation)"""
    ctx, k = lsd, 21
    deep = synth_reads(1500, read_len=150, genome_len=4000, sub_rate=0.01, seed=5, n_rate=0.002)
    shallow = synth_reads(300, read_len=150, genome_len=30000, sub_rate=0.01, seed=6, n_rate=0.002)
    reads = deep + shallow + ["", "ACGT", "ACGTTGCA" * 12, "N" * 80, "T" * 150]
    r = ctx.reads_from_ascii(reads)
    cset = ctx.count(r, k, B.CANONICAL | B.WITH_COUNTS)
    assert_lsd(ctx, "extract", "hist", "scatter", "unique")
    both, cnt = O.kmercount(reads, k, 16, 2, with_counts=True)
    mult = {tuple(row): int(c) for row, c in zip(both.tolist(), cnt.tolist())}
    for thr in (1, 3, 8):
        got = ctx.median_filter(r, cset, thr)
        exp = np.zeros(len(reads), dtype=np.uint8)
        for i, s in enumerate(reads):
            a, b = O.longest_valid(s)
            seg = s[a:b].upper()
            nk = len(seg) - k + 1
            if nk <= 0:
                continue
            m = sorted(mult[tuple(O.kmer_words(seg[p:p + k]))] for p in range(nk))
            exp[i] = 1 if m[nk // 2] >= thr else 0
        assert np.array_equal(got, exp), thr
        assert 0 < int(got.sum()) < len(reads)


@pytest.mark.parametrize("k", [21, 33])
def test_forced_extract_grid_stride(lsd, k):
    """more than 32 768 reads: launch_extract's grid (num_cus * 32 blocks of 4 waves) strides over the reads"""
    ctx = lsd
    n_waves = ctx.device_info()["num_cus"] * 32 * 4
    reads = synth_reads(40_000, read_len=150, genome_len=400_000, sub_rate=0.005, seed=400 + k)
    assert len(reads) > n_waves
    exp, expc = O.kmercount(reads, k, 16, 8, with_counts=True)
    s = ctx.count(ctx.reads_from_ascii(reads), k, B.BOTH_STRANDS | B.WITH_COUNTS)
    got, gotc = s.export(B.ORDER_REFERENCE_BUCKETS16, with_counts=True)
    assert_lsd(ctx, "extract", "expand", "hist", "scatter", "unique")
    assert np.array_equal(got, exp) and np.array_equal(gotc, expc)


# ---- b. edge sizes of the primitives ---------------------------------------------------------------------------------

@pytest.mark.parametrize("W,k", [(1, 27), (2, 45), (3, 81), (4, 121)])
def test_forced_sort_unique_edge_sizes(lsd, W, k):
    """n around one sort tile and one chunk of 256 tiles (the chunk base added by k_scatter / k_tile_offsets), random
    u32 counts (sums wrap), a pool of n/4 keys (runs for unique_records)"""
    ctx = lsd
    T = TILE[W]
    rng = np.random.default_rng(W)
    sizes = [1, 2, T - 1, T, T + 1, T * K_CHUNK - 1, T * K_CHUNK, T * K_CHUNK + 1, 3 * T * K_CHUNK + 17]
    for n in sizes:
        pool = random_keys(rng, max(1, n // 4), k)
        keys = pool[rng.integers(0, len(pool), size=n)]
        cnt = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
        ek, ec = expect_merge(keys, cnt)
        fams = ("hist", "scatter", "unique") if n > 1 else ("unique",)  # one record is sorted as it is
        s, _ = from_device(ctx, keys, k, cnt)
        gk, gc = s.export(B.ORDER_SORTED, with_counts=True)
        assert_lsd(ctx, *fams)
        assert len(s) == len(ek), n
        assert np.array_equal(gk, ek), n
        assert np.array_equal(gc, ec), n
        if n <= T + 1 or n == sizes[-1]:  # without counts: the same distinct set
            s2, _ = from_device(ctx, keys, k)
            assert np.array_equal(s2.export(B.ORDER_SORTED), ek), n
            assert_lsd(ctx, *fams)


@pytest.mark.parametrize("k", [31, 63])
def test_forced_runs_across_unique_tiles(lsd, k):
    """runs of equal keys against the 2048-record tiles of k_head_count / k_head_compact: one starting exactly on a tile
    boundary, one straddling one, and one key repeated 100 000 times (k_seg_reduce's serial loop)"""
    ctx = lsd
    rng = np.random.default_rng(k)
    mult = [1] * UNIQ_TILE + [100] + [1] * (4000 - UNIQ_TILE - 100) + [200] + [1] * 1000 + [100_000] + [1] * 500
    mult = np.array(mult, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(mult)[:-1]])
    assert starts[UNIQ_TILE] == UNIQ_TILE                                            # run on the boundary
    j = UNIQ_TILE + 1 + (4000 - UNIQ_TILE - 100)
    assert starts[j] < 2 * UNIQ_TILE < starts[j] + mult[j]                           # run across the next one
    distinct = random_keys(rng, 3 * len(mult), k)
    distinct = distinct[lex(distinct)]
    head = np.ones(len(distinct), dtype=bool)
    head[1:] = np.any(distinct[1:] != distinct[:-1], axis=1)
    distinct = distinct[head][:len(mult)]
    assert len(distinct) == len(mult)
    keys = np.repeat(distinct, mult, axis=0)
    cnt = rng.integers(0, 2**32, size=len(keys), dtype=np.uint64).astype(np.uint32)
    perm = rng.permutation(len(keys))
    keys, cnt = keys[perm], cnt[perm]
    ek, ec = expect_merge(keys, cnt)
    assert np.array_equal(ek, distinct)
    s, _ = from_device(ctx, keys, k, cnt)
    gk, gc = s.export(B.ORDER_SORTED, with_counts=True)
    assert_lsd(ctx, "hist", "scatter", "unique")
    assert np.array_equal(gk, ek) and np.array_equal(gc, ec)


@pytest.mark.parametrize("k", [32, 33, 64, 96, 127])
def test_forced_key_bits_at_pass_ends(lsd, k):
    """keys at the ends of key_passes' digits: the all-ones key (T x k; at k = 32 all 64 bits), keys differing only in
    the top bit of word 0 or only in the lowest bit of the last word, wide keys sharing word 0"""
    ctx = lsd
    nw = B.engine.words(k)
    rng = np.random.default_rng(500 + k)
    m = used_bits_mask(k)
    base = random_keys(rng, 3000, k)
    top0 = np.uint64(1 << (63 if nw > 1 else 2 * k - 1))
    hi = base[:200].copy()
    hi[:, 0] ^= top0
    lo = base[200:400].copy()
    lo[:, nw - 1] ^= np.uint64(1)
    special = [np.tile(m, (5, 1)), np.zeros((3, nw), dtype=np.uint64), hi, lo]
    if nw > 1:
        shared = random_keys(rng, 2000, k)
        shared[:, 0] = base[0, 0]
        special.append(shared)
    keys = np.concatenate([base, base[:500]] + special)
    keys = keys[rng.permutation(len(keys))]
    cnt = rng.integers(0, 2**32, size=len(keys), dtype=np.uint64).astype(np.uint32)
    ek, ec = expect_merge(keys, cnt)
    s, _ = from_device(ctx, keys, k, cnt)
    gk, gc = s.export(B.ORDER_SORTED, with_counts=True)
    assert_lsd(ctx, "hist", "scatter", "unique")
    assert np.array_equal(gk, ek) and np.array_equal(gc, ec)
    assert np.array_equal(gk[-1], m)  # the all-ones key is the largest


def test_forced_three_level_scan(lsd, monkeypatch):
    """more than 2048^2 reads: the k-mer offsets of dedup_reads go through a three-level exclusive_scan_u64; compared
    byte for byte with the default path"""
    ctx, k = lsd, 21
    n = 4_300_000
    assert n > SCAN_TILE * SCAN_TILE
    rng = np.random.default_rng(21)
    lens = rng.integers(k, k + 4, size=n).astype(np.uint32)      # k .. k+3 bases: one word per read
    words = rng.integers(0, 2**64, size=n, dtype=np.uint64, endpoint=False)
    words &= (np.uint64(1) << (2 * lens).astype(np.uint64)) - np.uint64(1)
    r = ctx.reads_from_packed(words, lens)
    s = ctx.count(r, k, B.CANONICAL | B.WITH_COUNTS)
    assert s.instances == int((lens - k + 1).sum())
    a, ac = s.export(B.ORDER_SORTED, with_counts=True)
    s.free()
    assert_lsd(ctx, "extract", "hist", "scatter", "unique")
    assert int(ac.sum(dtype=np.uint64)) == int((lens - k + 1).sum())
    d = msd_run(ctx, monkeypatch, lambda: ctx.count(r, k, B.CANONICAL | B.WITH_COUNTS))
    b, bc = d.export(B.ORDER_SORTED, with_counts=True)
    assert np.array_equal(a, b) and np.array_equal(ac, bc)


def test_forced_lsd_limit_refused(lsd):
    """a batch of more than 2^32 - 1 k-mer instances is refused after the one scan, never truncated"""
    ctx, k = lsd, 21
    n_reads = 33_100_000
    assert n_reads * (150 - k + 1) >= 2**32
    r = ctx.reads_synth(n_reads, read_len=150, genome_len=1_000_000)
    with pytest.raises(B.BBKError, match=r"LSD path is limited to 2\^32-1"):
        ctx.count(r, k, B.CANONICAL | B.WITH_COUNTS)
    assert launches(ctx, "extract") == 0 and launches(ctx, "hist") == 0
    r.free()
    assert_lsd(ctx)


# ---- one rule for count overflow ---------------------------------------------------------------------------------------

def _assert_count(keys, counts, key, want):
    i = np.flatnonzero(np.all(keys == key, axis=1))
    assert len(i) == 1
    assert int(counts[i[0]]) == want, "count %d, want %d (modulo 2^32)" % (int(counts[i[0]]), want)


@pytest.mark.parametrize("forced", [False, True], ids=["default", "lsd"])
def test_summed_counts_wrap(ctx, monkeypatch, forced):
    """key A x3 with 2^31 each -> 2^31; key B x2 with 2^32-1 each -> 2^32-2"""
    k = 21
    rng = np.random.default_rng(7)
    other = random_keys(rng, 5000, k)
    A, Bk = other[0].copy(), other[1].copy()
    other = other[2:]
    keys = np.concatenate([np.tile(A, (3, 1)), np.tile(Bk, (2, 1)), other])
    cnt = np.concatenate([np.full(3, 0x80000000, dtype=np.uint32), np.full(2, 0xFFFFFFFF, dtype=np.uint32),
                          rng.integers(1, 1000, size=len(other)).astype(np.uint32)])
    perm = rng.permutation(len(keys))
    keys, cnt = keys[perm], cnt[perm]
    if forced:
        monkeypatch.setenv("BBK_DISABLE_MSD", "1")
    ctx.profile(True)
    ctx.profile_reset()
    try:
        for flags in (0, B.UNSORTED):
            s, _ = from_device(ctx, keys, k, cnt, flags=flags)
            gk = np.zeros((len(s), 1), dtype=np.uint64)
            gc = np.zeros(len(s), dtype=np.uint32)
            s.export_by_owner(1, gk, gc)
            _assert_count(gk, gc, A, 0x80000000)
            _assert_count(gk, gc, Bk, 0xFFFFFFFE)
            ek, ec = expect_merge(keys, cnt)
            order = lex(gk)
            assert np.array_equal(gk[order], ek) and np.array_equal(gc[order], ec)
        assert_path(ctx, forced)
    finally:
        ctx.profile(False)
        ctx.profile_reset()


H_INSTANCES, H_COUNT = 20_000, 1 << 20
H_WANT = (H_INSTANCES * H_COUNT) % WRAP  # 20 971 520 000 mod 2^32 = 3 791 650 816 (saturating would give 2^32 - 1)


def heavy_key_input(rng, k=21, n_distinct=100_000):
    """n_distinct random keys (counts 1..999) beside key H repeated 20 000 times with 2^20 each"""
    other = random_keys(rng, n_distinct + 1, k)
    H = other[0].copy()
    other = other[1:]
    keys = np.concatenate([np.tile(H, (H_INSTANCES, 1)), other])
    cnt = np.concatenate([np.full(H_INSTANCES, H_COUNT, dtype=np.uint32),
                          rng.integers(1, 1000, size=len(other)).astype(np.uint32)])
    perm = rng.permutation(len(keys))
    return keys[perm], cnt[perm], H


def test_heavy_key_sum_wraps_on_lsd_path(lsd):
    ctx, k = lsd, 21
    keys, cnt, H = heavy_key_input(np.random.default_rng(8), k)
    s, _ = from_device(ctx, keys, k, cnt)
    gk, gc = s.export(B.ORDER_SORTED, with_counts=True)
    assert_lsd(ctx, "hist", "scatter", "unique")
    _assert_count(gk, gc, H, H_WANT)
    ek, ec = expect_merge(keys, cnt)
    assert np.array_equal(gk, ek) and np.array_equal(gc, ec)


@pytest.mark.parametrize("forced", [False, True], ids=["default", "lsd"])
def test_heavy_key_sum_wraps_through_a_merge(ctx, monkeypatch, forced):
    """key H split over two shard sets (each summing 10 000 x 2^20, already wrapped), exported with counts and merged
    again (the receive side of the owner exchange): the merged count is the same 3 791 650 816"""
    k = 21
    keys, cnt, H = heavy_key_input(np.random.default_rng(9), k, n_distinct=50_000)
    half = len(keys) // 2
    if forced:
        monkeypatch.setenv("BBK_DISABLE_MSD", "1")
    ctx.profile(True)
    ctx.profile_reset()
    parts_k, parts_c = [], []
    for a, b in ((0, half), (half, len(keys))):
        s, _ = from_device(ctx, keys[a:b], k, cnt[a:b], flags=B.UNSORTED)
        pk = np.zeros((len(s), 1), dtype=np.uint64)
        pc = np.zeros(len(s), dtype=np.uint32)
        s.export_by_owner(1, pk, pc)
        parts_k.append(pk)
        parts_c.append(pc)
    mk, mc = np.concatenate(parts_k), np.concatenate(parts_c)
    s, _ = from_device(ctx, mk, k, mc)
    gk, gc = s.export(B.ORDER_SORTED, with_counts=True)
    assert_path(ctx, forced)
    ctx.profile(False)
    _assert_count(gk, gc, H, H_WANT)
    ek, ec = expect_merge(keys, cnt)
    assert np.array_equal(gk, ek) and np.array_equal(gc, ec)


# ---- c. the fallbacks production takes at default knobs ---------------------------------------------------------------

FALLBACK_SCRIPT = r"""
import json, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch
import spades_for_blackbird_amd as B
from oracle import oracle as O
from tests.helpers import synth_reads
from tests.test_gpu_lsd_path import FAMS, lex, oracle_ext, heavy_key_input, from_device, expect_merge
ctx = B.Context(0, stream=torch.cuda.current_stream())
ctx.profile(True)
res = {}
def case(name, fn):
    sys.stderr.write("=== %%s\n" %% name)
    sys.stderr.flush()
    ctx.profile_reset()
    ok = bool(fn())
    res[name] = {"ok": ok, "fams": {f: ctx.profile_get(f)["launches"] for f in FAMS}}
    sys.stderr.write("=== end\n")
    sys.stderr.flush()
# one k-mer (poly-A) makes up ~60 %% of the instances: the MSD pass declines the whole call
reads = synth_reads(2000, read_len=150, genome_len=20000, sub_rate=0.005, seed=31) + ["A" * %(polya)d] * 3000
r = ctx.reads_from_ascii(reads)
for k in (21, 33):
    exp, expc = O.kmercount(reads, k, 16, 4, with_counts=True)
    def counts():
        g, gc = ctx.count(r, k, B.BOTH_STRANDS | B.WITH_COUNTS).export(B.ORDER_REFERENCE_BUCKETS16, with_counts=True)
        return np.array_equal(g, exp) and np.array_equal(gc, expc)
    def ref_order():
        return np.array_equal(ctx.count(r, k, B.BOTH_STRANDS | B.REFERENCE_ORDER).export(B.ORDER_REFERENCE_BUCKETS16), exp)
    def ext():
        ek, em = oracle_ext(reads, k)
        gk, gm = ctx.extindex(r, k).export()
        return np.array_equal(gk, ek) and np.array_equal(gm, em)
    case("decline_counts_%%d" %% k, counts)
    case("decline_ref_%%d" %% k, ref_order)
    case("decline_ext_%%d" %% k, ext)
# one key repeated 20 000 times beside 100 k distinct keys: its bucket is finished by sort_records + unique_records
keys, cnt, H = heavy_key_input(np.random.default_rng(8), 21)
def per_bucket():
    s, _ = from_device(ctx, keys, 21, cnt)
    gk, gc = s.export(B.ORDER_SORTED, with_counts=True)
    ek, ec = expect_merge(keys, cnt)
    i = np.flatnonzero(np.all(gk == H, axis=1))
    res["per_bucket_H"] = int(gc[i[0]]) if len(i) == 1 else -1
    return np.array_equal(gk, ek) and np.array_equal(gc, ec)
case("per_bucket", per_bucket)
ctx.close()
print(json.dumps(res))
"""
FAMS = LSD_FAMILIES + MSD_FAMILIES


def _segments(err):
    out, cur, name = {}, [], None
    for line in err.splitlines():
        if line.startswith("=== "):
            if name is not None:
                out[name] = "\n".join(cur)
            name = None if line == "=== end" else line[4:]
            cur = []
        elif name is not None:
            cur.append(line)
    return out


@pytest.mark.skipif(bool(os.environ.get("BBK_DISABLE_MSD")), reason="the fallbacks of the MSD path at default knobs")
def test_fallbacks_at_default_knobs():
    """A whole-call decline (poly-A at ~60 % of the instances; k = 21 and 33) and the per-bucket fallback of an
    oversized bucket, at default knobs in a fresh process with BBK_VERBOSE=1"""
    env = {kk: v for kk, v in os.environ.items() if not kk.startswith("BBK_") or kk == "BBK_LIB"}
    env["BBK_VERBOSE"] = "1"
    code = FALLBACK_SCRIPT % {"root": ROOT, "polya": 150}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    seg = _segments(out.stderr)
    for k in (21, 33):
        for what in ("counts", "ref", "ext"):
            name = "decline_%s_%d" % (what, k)
            assert res[name]["ok"], name
            assert "[bbk] msd declines:" in seg[name], (name, seg[name][-2000:])
            assert res[name]["fams"]["extract"] > 0, (name, res[name]["fams"])
    pb = res["per_bucket"]
    assert res["per_bucket_H"] == H_WANT
    assert pb["ok"]
    assert "[bbk] msd declines:" not in seg["per_bucket"], seg["per_bucket"][-2000:]
    lsd_buckets = [int(m) for m in re.findall(r" lsd=(\d+) \(", seg["per_bucket"])]
    assert lsd_buckets and max(lsd_buckets) >= 1, seg["per_bucket"][-2000:]
    assert sum(pb["fams"][f] for f in BUCKET_FAMILIES) > 0, pb["fams"]
    assert pb["fams"]["hist"] > 0 and pb["fams"]["scatter"] > 0 and pb["fams"]["unique"] > 0, pb["fams"]
