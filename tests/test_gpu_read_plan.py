"""The plan of the reads at the top of a count call: one fused scan over the read lengths, tile descriptors by lookup.

Every count from reads starts with a ReadPlan (bbk_internal.h): the k-mers of the reads (a total only), their units of
C k-mer positions (chunks of the level-1 kernels, super-k-mer segments) scanned into coff straight from the lengths, the
`unordered` flag of the packed words, and then one descriptor per tile of units (RdTile of the level-1 kernels, SkTile of
the super-k-mer path) found by an interpolated guess and a bounded gallop instead of a search over all reads.  The
test-only export bbk_read_plan brings all of that to the host, where it is compared field for field with numpy --
last_le's rule included: among equal coff entries the LAST owns the unit, so a unit behind a run of reads without k-mers
belongs to the read after the run.  The same read sets are then counted end to end against the oracle.

The read sets are built from lengths, not from a workload: random lengths 0..400 at n = 4095, 4096, 4097 (the edges of
a scan tile of 4096 items) and n = 70 001 (two scan levels); runs of reads shorter than k at the start, at the end and
exactly on a tile boundary; one read of 40 000 bases among 2000 and among 20 000 reads of 150 bp (several tile starts
inside one read; among 20 000 the guess behind it misses by more than the gallop covers, so the full bisection of the
rest takes over); reads that are all shorter than k.  Words that are not in read order come last, with one scan tile
and with a reduce pass, and with a single out-of-order pair across the edge of two workgroups.  Three scan levels need more than 4096^2 = 16.7 M reads and are not tested here.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RDTILE = np.dtype([("wbase", "<u8"), ("r0", "<u4"), ("nr", "<u4"), ("wspan", "<u4"), ("pad", "<u4")])
SKTILE = np.dtype([("r0", "<u4"), ("nr", "<u4")])
NO_STAGE = 0xFFFFFFFF
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def lib():
    L = B.load_library()
    L.bbk_read_plan_geometry.argtypes = [C.c_uint, C.POINTER(C.c_uint32)]
    L.bbk_read_plan_geometry.restype = C.c_int
    L.bbk_read_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_void_p,
                                C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64,
                                C.POINTER(C.c_uint64)]
    L.bbk_read_plan.restype = C.c_int
    return L


def geometry(k):
    """the kernels' own sizes at k"""
    g = (C.c_uint32 * 10)()
    assert lib().bbk_read_plan_geometry(k, g) == 0
    return dict(ch=g[0], scatter=g[1], hist=g[2], narrow=g[3], narrow_val=g[4], sk_c=g[5], sk_tile=g[6], slots=g[7],
                words=g[8])


# ---- read sets: (lengths, seed) -> bases -------------------------------------------------------------------

def lengths_of(name, k, C_, tile):
    """the lengths of read set `name` for k-mers of k in units of C_ and tiles of `tile` units"""
    one = k + C_ - 1  # a read of exactly one unit (C_ = 8: k + 7)
    if name.startswith("rand"):
        n = int(name[4:])
        return np.random.default_rng(n).integers(0, 401, size=n).astype(np.uint32)
    if name == "empty_start":
        return np.array([k - 1] * 37 + [150] * 700, dtype=np.uint32)
    if name == "empty_end":
        return np.array([150] * 700 + [k - 1] * 37 + [0] * 5, dtype=np.uint32)
    if name == "empty_boundary":  # the units of tile 1 start behind 50 reads that have none
        return np.array([one] * tile + [k - 1] * 50 + [one] * (tile // 2 + 3), dtype=np.uint32)
    if name == "long":
        lens = np.full(2001, 150, dtype=np.uint32)
        lens[777] = 40_000
        return lens
    if name == "long20k":  # behind the long read the even-spread guess is off by more than the gallop's 255 reads
        lens = np.full(20001, 150, dtype=np.uint32)
        lens[777] = 40_000
        return lens
    if name == "all_short":
        return np.random.default_rng(3).integers(0, k, size=5000).astype(np.uint32)
    raise KeyError(name)


SETS = ["rand4095", "rand4096", "rand4097", "rand70001", "empty_start", "empty_end", "empty_boundary", "long", "long20k",
        "all_short"]
_blobs = {}


def blob_of(lens, seed=1):
    """random bases for reads of the given lengths: (bytes, offsets u64[n + 1]); cached"""
    key = (lens.tobytes(), seed)
    if key not in _blobs:
        offs = np.zeros(len(lens) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(lens, dtype=np.uint64)
        codes = np.random.default_rng(seed).integers(0, 4, size=int(offs[-1]), dtype=np.uint8)
        _blobs[key] = (LUT[codes].tobytes(), offs)
    return _blobs[key]


# ---- the plan in numpy --------------------------------------------------------------------------------------------

def plan_ref(lens, woff, k, C_, tile, superk, unordered, geo):
    lens = lens.astype(np.int64)
    n = len(lens)
    kmers = np.maximum(0, lens - k + 1)
    units = -(-kmers // C_)
    coff = np.zeros(n + 1, dtype=np.int64)
    coff[1:] = np.cumsum(units)
    U = int(coff[n])
    nt = -(-U // tile)
    c0 = np.arange(nt, dtype=np.int64) * tile

    def last_le(x):  # largest r in [0, n) with coff[r] <= x
        return np.searchsorted(coff[:n], x, side="right") - 1
    r0 = last_le(c0)
    if superk:
        r1 = last_le(np.minimum(c0 + tile, U) - 1)
        t = np.zeros(nt, dtype=SKTILE)
        t["r0"], t["nr"] = r0, r1 - r0 + 1
        return coff, int(kmers.sum()), U, t
    r1 = last_le(c0 + tile)
    woff = woff.astype(np.int64)
    p0 = (c0 - coff[r0]) * C_
    wbase = woff[r0] + (np.where(p0 > 0, p0 - 1, 0) >> 5)
    len1 = lens[r1]
    span1 = (c0 + tile - coff[r1]) * C_ + k
    lastb1 = np.where(len1 > 0, np.minimum(span1, len1 - 1), 0)
    wend = woff[r1] + np.where(len1 > 0, (lastb1 >> 5) + 1, 0)
    nr = r1 - r0 + 1
    fast = (not unordered) & (nr <= geo["slots"]) & (wend >= wbase) & (wend - wbase <= geo["words"])
    t = np.zeros(nt, dtype=RDTILE)
    t["wbase"], t["r0"], t["nr"] = wbase, r0, nr
    t["wspan"] = np.where(fast, wend - wbase, NO_STAGE)
    return coff, int(kmers.sum()), U, t


def plan_gpu(ctx, reads, n, k, C_, tile, superk):
    coff = np.zeros(n + 1, dtype=np.uint64)
    tot = (C.c_uint64 * 2)()
    flag = C.c_uint32(7)
    cap = 1 << 16
    tiles = np.zeros(cap, dtype=SKTILE if superk else RDTILE)
    nt = C.c_uint64(0)
    rc = lib().bbk_read_plan(ctx._h, reads._h, k, C_, tile, int(superk), coff.ctypes.data, tot, C.byref(flag),
                             tiles.ctypes.data, cap, C.byref(nt))
    assert rc == 0, lib().bbk_last_error()
    return coff.astype(np.int64), int(tot[0]), int(tot[1]), int(flag.value), tiles[:nt.value]


def plan_cases():
    """(k, C, tile, superk) for every tiling the kernels use: (21, 8), (31, 8), (55, 4) with the scatter, histogram and
    narrow tiles of the level-1 kernels, and k = 55 in super-k-mer segments"""
    out = []
    for k in (21, 31, 55):
        g = geometry(k)
        assert g["ch"] == {21: 8, 31: 8, 55: 4}[k]
        for tile in sorted({g["scatter"], g["hist"], g["narrow"]}):
            out.append((k, g["ch"], tile, False))
    g = geometry(55)
    assert g["sk_c"] >= 1
    out.append((55, g["sk_c"], g["sk_tile"], True))
    return out


def check_plan(ctx, name, k, C_, tile, superk):
    lens = lengths_of(name, k, C_, tile)
    n = len(lens)
    blob, offs = blob_of(lens)
    reads = ctx.reads_from_blob(blob, offs)
    try:
        woff = np.zeros(n + 1, dtype=np.int64)  # every read starts on a word, in read order
        woff[1:] = np.cumsum((lens.astype(np.int64) + 31) >> 5)
        ecoff, ekm, eu, etiles = plan_ref(lens, woff, k, C_, tile, superk, False, geometry(k))
        coff, km, u, flag, tiles = plan_gpu(ctx, reads, n, k, C_, tile, superk)
        what = (name, k, C_, tile, superk)
        assert (km, u, flag) == (ekm, eu, 0), what
        assert np.array_equal(coff, ecoff), (what, np.flatnonzero(coff != ecoff)[:8])
        assert len(tiles) == len(etiles), what
        for f in etiles.dtype.names:
            bad = np.flatnonzero(tiles[f] != etiles[f])
            assert len(bad) == 0, (what, f, bad[:8], tiles[bad[:8]], etiles[bad[:8]])
        return etiles, ecoff
    finally:
        reads.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_plan_against_numpy(ctx, name):
    """coff, both totals, the flag and every field of every tile descriptor, for every tiling the kernels use"""
    for k, C_, tile, superk in plan_cases():
        etiles, ecoff = check_plan(ctx, name, k, C_, tile, superk)
        if name == "all_short":
            assert len(etiles) == 0 and ecoff[-1] == 0
        if name == "empty_boundary":  # tile 1 starts behind the 50 empty reads: the LAST of the equal entries owns it
            assert etiles["r0"][1] == tile + 50, (k, C_, tile)
            # tile 0 ends on the read that holds unit `tile` (RdTile: exclusive end) or on its own last read (SkTile)
            assert etiles["nr"][0] == (tile if superk else tile + 51), (k, C_, tile, etiles[0])
        if name in ("long", "long20k"):  # more than one tile starts inside the long read
            assert np.count_nonzero(etiles["r0"] == 777) >= 2, (k, C_, tile)


# ---- end to end ------------------------------------------------------------------------------------------------------

FLAGS = B.BOTH_STRANDS | B.REFERENCE_ORDER
_oracle = {}


def oracle_count(name, k, lens):
    if (name, k) not in _oracle:
        blob, offs = blob_of(lens)
        _oracle[(name, k)] = O.kmercount(None, k, 16, 4, blob=O.mk_reads_blob(blob, offs))
    return _oracle[(name, k)]


def e2e_lengths(name, k):
    """the set of the plan test at the chunking of the path k takes (k = 55: super-k-mer segments)"""
    g = geometry(k)
    if k == 55:
        return lengths_of(name, k, g["sk_c"], g["sk_tile"])
    return lengths_of(name, k, g["ch"], g["narrow"] if k == 21 else g["scatter"])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 31, 55])
@pytest.mark.parametrize("name", SETS)
def test_count_equals_oracle(ctx, name, k):
    """k = 21: the narrow path; k = 31: 8-byte keys from reads; k = 55: super-k-mers"""
    lens = e2e_lengths(name, k)
    blob, offs = blob_of(lens)
    reads = ctx.reads_from_blob(blob, offs)
    try:
        s = ctx.count(reads, k, FLAGS)
        got = s.export(B.ORDER_REFERENCE_BUCKETS16)
        exp = oracle_count(name, k, lens)
        if name == "all_short":
            assert len(got) == 0 and len(exp) == 0
        assert got.shape == exp.shape and np.array_equal(got, exp), (name, k, got.shape, exp.shape)
        s.free()
    finally:
        reads.free()


LSD_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import spades_for_blackbird_amd as B
from tests import test_gpu_read_plan as T
ctx = B.Context(0)
ctx.profile(True)
for name in T.SETS:
    lens = T.e2e_lengths(name, 21)
    blob, offs = T.blob_of(lens)
    reads = ctx.reads_from_blob(blob, offs)
    ctx.profile_reset()
    got = ctx.count(reads, 21, T.FLAGS).export(B.ORDER_REFERENCE_BUCKETS16)
    exp = T.oracle_count(name, 21, lens)
    assert got.shape == exp.shape and np.array_equal(got, exp), (name, got.shape, exp.shape)
    if len(exp):
        assert ctx.profile_get("extract")["launches"] > 0, name
print("LSD-OK")
"""


@pytest.mark.gpu
def test_count_equals_oracle_on_the_general_path():
    """k = 21 once more with BBK_DISABLE_MSD=1 in a child process: the plan in units of one k-mer feeds k_extract"""
    env = dict(os.environ, BBK_DISABLE_MSD="1")
    r = subprocess.run([sys.executable, "-c", LSD_SCRIPT % {"root": ROOT}], capture_output=True, text=True, env=env,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "LSD-OK" in r.stdout


def pack_reads(lens, codes, order):
    """2-bit packed reads, every read on a word boundary, the words of read order[0] first: (words, woff)"""
    n = len(lens)
    L = lens.astype(np.int64)
    nw = (L + 31) >> 5
    start = np.zeros(n + 1, dtype=np.int64)
    start[1:] = np.cumsum(L)
    wnat = np.zeros(n + 1, dtype=np.int64)  # first word of every read when the words lie in read order
    wnat[1:] = np.cumsum(nw)
    padded = np.zeros(int(wnat[n]) * 32, dtype=np.uint64)
    padded[np.arange(int(start[n])) + np.repeat(wnat[:n] * 32 - start[:n], L)] = codes
    nat = (padded.reshape(-1, 32) << (2 * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    order = np.asarray(order, dtype=np.int64)
    woff = np.zeros(n + 1, dtype=np.int64)
    woff[order] = np.concatenate([[0], np.cumsum(nw[order])[:-1]])
    woff[n] = wnat[n]
    words = np.zeros(int(wnat[n]), dtype=np.uint64)
    words[np.arange(int(wnat[n])) + np.repeat(woff[:n] - wnat[:n], nw)] = nat
    return words, woff.astype(np.uint64)


def out_of_order_pairs(lens, woff):
    """the reads i whose successor's words start before their own end (what sets the flag)"""
    w = woff.astype(np.int64)
    return np.flatnonzero(w[1:-1] < w[:-2] + ((lens[:-1].astype(np.int64) + 31) >> 5))


# One scan tile holds 4096 reads.  3001 reads: the scan is its one top workgroup, which then checks the word order itself;
# 9001 reads: the check runs in the reduce pass (three workgroups) as in every real call.  "reversed": the words of the
# reads lie back to front, nearly every pair is out of order; "pair": the words lie in read order except that those of
# read 4096 come before those of read 4095 -- ONE pair is out of order, and it straddles two workgroups of the reduce pass
@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 55])
@pytest.mark.parametrize("layout,n", [("reversed", 3001), ("reversed", 9001), ("pair", 9001)])
def test_words_not_in_read_order(ctx, layout, n, k):
    """reads_from_device with words that are not in read order: the flag is set, no tile stages its words (every wspan
    is the marker), every other field is as in numpy, and the count equals the oracle"""
    import torch
    rng = np.random.default_rng(17)
    lens = rng.integers(0, 301, size=n).astype(np.uint32)
    if layout == "pair":
        lens[4095:4097] = 150
        order = np.arange(n)
        order[4095:4097] = (4096, 4095)
    else:
        order = np.arange(n - 1, -1, -1)
    codes = rng.integers(0, 4, size=int(lens.sum()), dtype=np.uint8)
    words, woff = pack_reads(lens, codes, order)
    bad = out_of_order_pairs(lens, woff)
    if layout == "pair":
        assert bad.tolist() == [4095]
    else:
        assert len(bad) > n // 2
    dw = torch.from_numpy(words.view(np.int64)).cuda()
    do = torch.from_numpy(woff.view(np.int64)).cuda()
    dl = torch.from_numpy(lens.view(np.int32)).cuda()
    torch.cuda.synchronize()
    reads = ctx.reads_from_device(dw, do, dl, n, len(words))
    g = geometry(k)
    tile = g["narrow"] if k == 21 else g["scatter"]
    ecoff, ekm, eu, etiles = plan_ref(lens, woff[:-1].astype(np.int64), k, g["ch"], tile, False, True, g)
    coff, km, u, flag, tiles = plan_gpu(ctx, reads, n, k, g["ch"], tile, False)
    assert flag == 1 and (km, u) == (ekm, eu)
    assert np.array_equal(coff, ecoff)
    assert len(tiles) and np.all(tiles["wspan"] == NO_STAGE)
    for f in ("wbase", "r0", "nr", "wspan", "pad"):
        assert np.array_equal(tiles[f], etiles[f]), f
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens, dtype=np.uint64)
    exp = O.kmercount(None, k, 16, 4, blob=O.mk_reads_blob(LUT[codes].tobytes(), offs))
    s = ctx.count(reads, k, FLAGS)
    got = s.export(B.ORDER_REFERENCE_BUCKETS16)
    assert got.shape == exp.shape and np.array_equal(got, exp), (layout, n, k, got.shape, exp.shape)
    s.free()
    reads.free()


def test_read_plan_entry_points_are_exported():
    """no GPU: the library carries the two test exports and the plan's kernels, and none of them uses scratch"""
    from spades_for_blackbird_amd import build as b
    L = C.CDLL(b.build())
    assert hasattr(L, "bbk_read_plan") and hasattr(L, "bbk_read_plan_geometry")
    res = b.check_resources()
    if res is not None:
        names = " ".join(r[1] for r in res)
        for kern in ("k_tile_reads", "k_sk_tiles", "k_scan_reduce", "k_scan_apply"):
            assert kern in names, kern
        for gone in ("k_kmers_per_read", "k_sk_segments"):
            assert gone not in names, gone
