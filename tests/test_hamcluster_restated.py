"""CPU: the restatement of the reference's tau = 1 Hamming clustering (tests/hamcluster_restated.py) against a brute-force
component finder, and the two facts the engine's split between device and host rests on: below the lock
size a cluster is a plain component, and the components of lock_size members or more can be replayed alone."""
import numpy as np
import pytest

from tests import hamcluster_restated as R

KS = [5, 6, 20, 21, 31, 32]


def read_keys(k, seed, n_reads=12, read_len=100, genome_len=400, sub_rate=0.03):
    """the rc-closed ascending k-mer set of reads with substitutions (one-word keys as python ints)"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, genome_len)
    keys = set()
    for st in rng.integers(0, genome_len - read_len + 1, n_reads):
        r = g[st:st + read_len].copy()
        sub = rng.random(read_len) < sub_rate
        r[sub] = (r[sub] + rng.integers(1, 4, int(sub.sum()))) & 3
        for p in range(read_len - k + 1):
            keys.add(sum(int(b) << (2 * i) for i, b in enumerate(r[p:p + k])))
    return R.both_strands(keys, k)


def test_rc_and_dsu_by_hand():
    assert R.rc(R.encode("ACGTT"), 5) == R.encode("AACGT")
    assert R.rc(R.encode("ACGT"), 4) == R.encode("ACGT")
    uf = R.DSU(4)
    uf.unite(0, 1)  # equal sizes: the lower index goes under the higher
    assert uf.find_set(0) == 1 and uf.set_size(0) == 2
    uf.set_root_aux(2, R.FULLY_LOCKED)
    uf.unite(2, 0)  # the larger set stays root and keeps its aux
    assert uf.find_set(2) == 1 and uf.root_aux(2) == R.UNLOCKED and uf.set_size(2) == 3
    uf.set_root_aux(3, R.FULLY_LOCKED)
    assert not R.can_merge(uf, 0, 3) and R.can_merge(uf, 0, 2)


@pytest.mark.parametrize("k", KS)
def test_without_lock_the_clusters_are_the_components(k):
    keys = read_keys(k, seed=k)
    assert len(keys) > 300
    lab = R.labels_list(R.cluster(keys, k, lock_size=len(keys) + 1), len(keys))
    comp = R.components(keys, k)
    assert lab == comp
    assert len(set(comp)) < len(keys)  # something was united
    lab2, replayed = R.with_replay(keys, k, lock_size=len(keys) + 1)
    assert lab2 == comp and replayed == 0


@pytest.mark.parametrize("k", KS)
def test_oversize_components_can_be_replayed_alone(k):
    keys = read_keys(k, seed=100 + k, n_reads=40, read_len=50, genome_len=120)  # ~16x: components of 6 at every k
    full = R.labels_list(R.cluster(keys, k, lock_size=6, chunk=16), len(keys))
    lab, replayed = R.with_replay(keys, k, lock_size=6, chunk=16)
    assert lab == full
    assert replayed > 0
    if k < 7:  # one big component: the lock changes the result
        assert len(set(full)) > len(set(R.components(keys, k)))


def test_listing_and_files():
    members, sizes = R.listing([0, 1, 0, 3, 1, 0])
    assert members == [0, 2, 5, 1, 4, 3] and sizes == [3, 2, 1]
    a, b = R.file_bytes([0, 1, 0, 3, 1, 0])
    assert np.frombuffer(a, dtype=np.uint64).tolist() == members and np.frombuffer(b, dtype=np.uint64).tolist() == sizes
