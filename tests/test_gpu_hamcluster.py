"""GPU: Hamming-graph clustering of a both-strand k-mer set (KMerSet.hamming_clusters, spades-hamcluster) against the
literal restatement of the reference's chunked rule (tests/hamcluster_restated.py): labels, members and sizes byte for
byte.  The restatement runs over the whole set; the engine finds the plain components on the device and replays only
those of lock_size members or more on the host."""
import os
import subprocess

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build_host
from tests import hamcluster_restated as R
from tests.helpers import rc as rc_str

pytestmark = pytest.mark.gpu

KS = [5, 6, 20, 21, 31, 32]


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def _reads(rng, genome, n, read_len=100, sub_rate=0.03):
    out = []
    for st in rng.integers(0, len(genome) - read_len + 1, n):
        r = list(genome[st:st + read_len])
        for j in np.nonzero(rng.random(read_len) < sub_rate)[0]:
            r[j] = "ACGT"[("ACGT".index(r[j]) + int(rng.integers(1, 4))) & 3]
        r = "".join(r)
        out.append(rc_str(r) if rng.random() < 0.5 else r)
    return out


@pytest.fixture(scope="module")
def read_set(ctx):
    """k -> (KMerSet, its keys as python ints) of 300 x 100 bp reads with 3 % substitutions; built once per k"""
    sets = {}

    def get(k):
        if k not in sets:
            rng = np.random.default_rng(1000 + k)
            genome = "".join(rng.choice(list("ACGT"), 600))
            s = ctx.count(ctx.reads_from_ascii(_reads(rng, genome, 300)), k, B.BOTH_STRANDS)
            sets[k] = (s, [int(x) for x in s.export()[:, 0]])
        return sets[k]

    yield get
    for s, _ in sets.values():
        s.free()


def _canonical(key, k):
    """the strand a canonical set keeps: base 0 first"""
    r = R.rc(key, k)
    a = [(key >> (2 * i)) & 3 for i in range(k)]
    b = [(r >> (2 * i)) & 3 for i in range(k)]
    return key if a <= b else r


def _set_of(ctx, keys, k):
    """(both-strand KMerSet, its keys) from any list of one-word keys, through kmerset_from_device + both_strands"""
    import torch
    canon = np.array(sorted({_canonical(int(x), k) for x in keys}), dtype=np.uint64)
    d = torch.from_numpy(canon.view(np.int64)).cuda()
    torch.cuda.synchronize()
    s = ctx.kmerset_from_device(d, len(canon), k).both_strands()
    exp = R.both_strands(keys, k)
    assert [int(x) for x in s.export()[:, 0]] == exp
    return s, exp


def _check(h, labels):
    """every output of the engine == what the labels of the restatement give"""
    members, sizes = R.listing(labels)
    assert h.size == len(labels) and len(h) == len(sizes)
    assert h.labels().tobytes() == np.array(labels, dtype=np.uint64).tobytes()
    assert h.members().tobytes() == np.array(members, dtype=np.uint64).tobytes()
    assert h.sizes().tobytes() == np.array(sizes, dtype=np.uint64).tobytes()


def _restated(keys, k, lock_size=R.LOCK_SIZE, chunk=R.CHUNK):
    return R.labels_list(R.cluster(keys, k, lock_size, chunk), len(keys))


@pytest.mark.parametrize("k", KS)
def test_reads_with_substitutions(read_set, tmp_path, k):
    s, keys = read_set(k)
    h = s.hamming_clusters()
    labels = _restated(keys, k)
    _check(h, labels)
    assert len(set(labels)) < len(keys)
    if k >= 20:
        assert h.replayed == 0
    # the files: ConcurrentDSU::extract_to_file
    path = str(tmp_path / "kmers.hamming")
    h.write(path)
    exp_members, exp_sizes = R.file_bytes(labels)
    assert open(path, "rb").read() == exp_members and open(path + ".idx", "rb").read() == exp_sizes
    h.close()
    h.close()


@pytest.mark.parametrize("k", [5, 6])
def test_lock_path_small_k(read_set, k):
    """lock_size = 6, chunk = 16: nearly everything is replayed, and the lock changes the result"""
    s, keys = read_set(k)
    h = s.hamming_clusters(lock_size=6, chunk=16)
    labels = _restated(keys, k, 6, 16)
    _check(h, labels)
    assert h.replayed > 0
    comp = R.components(keys, k)
    assert labels != comp and len(set(labels)) > len(set(comp))
    _check(s.hamming_clusters(lock_size=len(keys) + 1), comp)  # no lock: the plain components


def _random_kmers(rng, n, k):
    return [int(rng.integers(0, 1 << 62)) & ((1 << (2 * k)) - 1) for _ in range(n)]


def _sub(key, pos, delta=1):
    base = (key >> (2 * pos)) & 3
    return (key & ~(3 << (2 * pos))) | (((base + delta) & 3) << (2 * pos))


def test_crafted_pairs(ctx):
    k = 21
    rng = np.random.default_rng(5)
    base = _random_kmers(rng, 50, k)
    a, b, c, d = base[:4]
    top = _sub(a, k - 1)        # differs from a only at base k - 1: found only through the mirror block
    mid = _sub(b, k // 2)       # differs from b only at base floor(k / 2)
    low = _sub(c, 0, 2)         # differs from c only at base 0
    two = _sub(_sub(d, 3), 17)  # distance 2 from d: stays apart
    s, keys = _set_of(ctx, base + [top, mid, low, two], k)
    h = s.hamming_clusters()
    labels = _restated(keys, k)
    assert labels == R.components(keys, k)
    _check(h, labels)
    lab = dict(zip(keys, labels))
    for x, y in ((a, top), (b, mid), (c, low)):
        assert lab[x] == lab[y] and lab[R.rc(x, k)] == lab[R.rc(y, k)] and lab[x] != lab[R.rc(x, k)]
    assert lab[d] != lab[two]
    assert len(set(labels)) == len(keys) - 6 and h.replayed == 0


def test_crafted_palindrome(ctx):
    k = 20
    rng = np.random.default_rng(6)
    half = "".join(rng.choice(list("ACGT"), k // 2))
    pal = R.encode(half + rc_str(half))
    assert R.rc(pal, k) == pal
    nb = _sub(pal, 4)  # its reverse complement differs from the palindrome at base k - 1 - 4
    base = _random_kmers(rng, 40, k)
    s, keys = _set_of(ctx, base + [pal, nb], k)
    assert len(keys) == 2 * 40 + 3
    h = s.hamming_clusters()
    labels = _restated(keys, k)
    assert labels == R.components(keys, k)
    _check(h, labels)
    lab = dict(zip(keys, labels))
    assert lab[pal] == lab[nb] == lab[R.rc(nb, k)]
    assert sorted(h.sizes().tolist())[-1] == 3


@pytest.fixture(scope="module")
def long_block(ctx):
    """all 4^6 completions of the low six bases under fixed upper bases at k = 21: 4096 consecutive records of one
    block, and their reverse complements; unrelated records in front so the block starts inside a tile"""
    k = 21
    rng = np.random.default_rng(7)
    upper = int(rng.integers(0, 1 << 30)) | (3 << 28)  # 15 bases, the top one T: unrelated records sort before it
    block = [(upper << 12) | low for low in range(4096)]
    s, keys = _set_of(ctx, block + _random_kmers(rng, 75, k), k)
    first = keys.index(block[0])
    assert keys[first:first + 4096] == block and first % 256 != 0
    yield k, s, keys, R.components(keys, k), first
    s.free()


@pytest.mark.parametrize("lock_size,chunk", [(0, 0), (5000, 0), (1000, 32)])
def test_one_long_block(ctx, long_block, lock_size, chunk):
    """With the default lock size the restatement itself does not split this block at any chunk size tried (16 to
    65536): the components go through the replay and come out whole.  lock_size = 1000, chunk = 32 is the case in which
    the lock splits them."""
    k, s, keys, comp, first = long_block
    assert sorted(R.listing(comp)[1])[-2:] == [4096, 4096]  # the block and its reverse complements
    assert len(set(comp[first:first + 4096])) == 1
    h = s.hamming_clusters(lock_size=lock_size, chunk=chunk)
    labels = _restated(keys, k, lock_size or R.LOCK_SIZE, chunk or R.CHUNK)
    _check(h, labels)
    if lock_size == 5000:  # below the lock size: nothing replayed
        assert h.replayed == 0 and labels == comp
    elif lock_size == 0:  # 4096 >= 2500: replayed
        assert h.replayed == 8192 and labels == comp
    else:
        assert h.replayed == 8192 and labels != comp and len(set(labels)) > len(set(comp))


def test_refusals(ctx):
    import torch
    k = 21
    reads = ctx.reads_synth(300, read_len=100, genome_len=1500)
    good = ctx.count(reads, k, B.BOTH_STRANDS)
    with pytest.raises(B.BBKError, match="tau > 1 not built"):
        good.hamming_clusters(tau=2)
    with pytest.raises(B.BBKError, match="k <= 32"):
        ctx.count(reads, 33, B.BOTH_STRANDS).hamming_clusters()
    with pytest.raises(B.BBKError, match="final_kmers order"):
        ctx.count(reads, k, B.BOTH_STRANDS | B.REFERENCE_ORDER).hamming_clusters()
    d = torch.from_numpy(good.export().view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    with pytest.raises(B.BBKError, match="BBK_UNSORTED"):
        ctx.kmerset_from_device(d, len(good), k, flags=B.UNSORTED).hamming_clusters()
    with pytest.raises(B.BBKError, match="not closed under reverse complement"):
        ctx.count(reads, k, B.CANONICAL).hamming_clusters()
    try:
        good.hamming_clusters(tau=0)
    except B.BBKError as e:
        assert "bbk error -1" in str(e)  # BBK_ERR_ARG
    else:
        raise AssertionError("tau = 0 was accepted")
    empty = ctx.count(ctx.reads_from_ascii(["ACGT"]), k, B.BOTH_STRANDS)
    h = empty.hamming_clusters()
    assert len(empty) == 0 and len(h) == 0 and h.size == 0 and h.replayed == 0
    assert h.labels().size == 0 and h.members().size == 0 and h.sizes().size == 0
    assert len(good.hamming_clusters()) > 0  # the context is still usable


def test_tool(ctx, golden_dir, tmp_path):
    bins = {os.path.basename(p): p for p in build_host.build()}
    k = 21
    fq = os.path.join(golden_dir, "ecoli_1K_1.fq.gz")
    prefix = str(tmp_path / "out")
    r = subprocess.run([bins["spades-hamcluster"], "-k", str(k), "-t", "2", "-b", "100000", "-o", prefix, fq],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    from tests.helpers import read_fastq_gz
    exp = ctx.count(ctx.reads_from_ascii(read_fastq_gz(fq)), k, B.BOTH_STRANDS).export()
    assert open(prefix + ".kmers", "rb").read() == exp.tobytes()
    keys = [int(x) for x in exp[:, 0]]
    labels = _restated(keys, k)
    members, sizes = R.file_bytes(labels)
    assert open(prefix + ".hamming", "rb").read() == members
    assert open(prefix + ".hamming.idx", "rb").read() == sizes
    n_sizes = R.listing(labels)[1]
    assert "%d k-mers, %d clusters, largest cluster %d, replayed k-mers 0" % (len(keys), len(n_sizes), max(n_sizes)) in r.stdout
    r = subprocess.run([bins["spades-hamcluster"], "-k", "33", "-o", prefix, fq], capture_output=True, text=True)
    assert r.returncode != 0 and "out of range" in r.stderr
    r = subprocess.run([bins["spades-hamcluster"], fq], capture_output=True, text=True)
    assert r.returncode == 1 and "SYNOPSIS" in r.stdout
