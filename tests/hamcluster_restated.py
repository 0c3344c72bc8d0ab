"""Literal sequential restatement (pure Python, no GPU, no reference code) of BayesHammer's tau = 1 Hamming clustering
for the tests of the Hamming-cluster engine:

  * TauOneKMerHamClusterer::cluster / ClusterChunk / canMerge2 (projects/hammer/hamcluster.cpp:207-289): chunks of
    indices, 3k substitutions of one k-mer of every strand pair, no union with a locked set, the second union (of the two
    reverse complements) without a lock check, the lock pass after every chunk;
  * dsu::ConcurrentDSU::unite (common/adt/concurrent_dsu.hpp:46-96): the smaller set goes under the larger, of two equal
    ones the lower index under the higher, the root that stays keeps its aux;
  * ConcurrentDSU::extract_to_file (concurrent_dsu.cpp:17-86): the member indices cluster by cluster, then the sizes.

What is the engine's and not the reference's: an index is a position in the ascending set (one-word keys,
k <= 32, base i in bits 2i), the processed strand of a pair is the one with key <= rc(key), and clusters are labelled by
and listed in the order of their smallest member.  Plus a brute-force all-pairs component finder.
"""
import numpy as np

UNLOCKED, FULLY_LOCKED = 0, 3
LOCK_SIZE, CHUNK = 2500, 64 * 1024


def rc(key, k):
    """reverse complement of a one-word key"""
    r = 0
    for i in range(k):
        r |= (3 - ((key >> (2 * i)) & 3)) << (2 * (k - 1 - i))
    return r


def encode(kmer):
    return sum("ACGT".index(c) << (2 * i) for i, c in enumerate(kmer))


def both_strands(keys, k):
    """ascending rc-closed set of python ints"""
    s = set(int(x) for x in keys)
    return sorted(s | {rc(x, k) for x in s})


class DSU:
    def __init__(self, n):
        self.parent = list(range(n))
        self.size = [1] * n
        self.aux = [UNLOCKED] * n

    def find_set(self, x):
        r = x
        while self.parent[r] != r:
            r = self.parent[r]
        while self.parent[x] != r:
            self.parent[x], x = r, self.parent[x]
        return r

    def unite(self, x, y):
        x, y = self.find_set(x), self.find_set(y)
        if x == y:
            return
        if self.size[x] > self.size[y] or (self.size[x] == self.size[y] and x > y):
            x, y = y, x
        self.parent[x] = y  # y keeps its aux
        self.size[y] += self.size[x]

    def set_size(self, x):
        return self.size[self.find_set(x)]

    def root_aux(self, x):
        return self.aux[self.find_set(x)]

    def set_root_aux(self, x, v):
        self.aux[self.find_set(x)] = v


def can_merge(uf, a, b):
    return uf.root_aux(a) != FULLY_LOCKED and uf.root_aux(b) != FULLY_LOCKED


def cluster(keys, k, lock_size=LOCK_SIZE, chunk=CHUNK, subset=None):
    """keys: the ascending rc-closed set (python ints).  subset: ascending global indices to run the rule on alone (they
    keep their global indices for the chunk boundaries); None = all.  Returns {global index: label}, label = smallest
    global index of the cluster."""
    idx = list(range(len(keys))) if subset is None else list(subset)
    local = {keys[g]: j for j, g in enumerate(idx)}
    uf = DSU(len(idx))
    j = 0
    while j < len(idx):
        c = idx[j] // chunk
        e = j
        while e < len(idx) and idx[e] // chunk == c:
            e += 1
        for x in range(j, e):
            kmer = keys[idx[x]]
            rk = rc(kmer, k)
            if kmer > rk:
                continue
            rcx = None
            for p in range(k):
                cur = (kmer >> (2 * p)) & 3
                for nc in range(4):
                    if nc == cur:
                        continue
                    cand = (kmer & ~(3 << (2 * p))) | (nc << (2 * p))
                    y = local.get(cand)
                    if y is not None and can_merge(uf, x, y):
                        uf.unite(x, y)
                        if rcx is None:
                            rcx = local[rk]
                        uf.unite(rcx, local[rc(cand, k)])
        for x in range(j, e):
            if uf.set_size(x) < lock_size:
                continue
            if uf.root_aux(x) != FULLY_LOCKED:
                uf.set_root_aux(x, FULLY_LOCKED)
        j = e
    low = {}
    out = {}
    for x, g in enumerate(idx):
        out[g] = low.setdefault(uf.find_set(x), g)
    return out


def components(keys, k):
    """brute force: labels (smallest member) of the connected components of the Hamming-1 graph, all pairs compared"""
    a = np.array(keys, dtype=np.uint64)
    n = len(a)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    m = np.uint64(0x5555555555555555)
    for i in range(n - 1):
        x = a[i + 1:] ^ a[i]
        x = (x | (x >> np.uint64(1))) & m
        one = (x != 0) & ((x & (x - np.uint64(1))) == 0)
        for j in np.nonzero(one)[0]:
            ri, rj = find(i), find(i + 1 + int(j))
            if ri != rj:
                parent[max(ri, rj)] = min(ri, rj)
    return [find(i) for i in range(n)]


def labels_list(lab, n):
    return [lab[i] for i in range(n)]


def listing(labels):
    """(members, sizes): indices grouped by label, clusters by ascending label, ascending inside a cluster"""
    groups = {}
    for i, l in enumerate(labels):
        groups.setdefault(l, []).append(i)
    members, sizes = [], []
    for l in sorted(groups):
        members += groups[l]
        sizes.append(len(groups[l]))
    return members, sizes


def with_replay(keys, k, lock_size=LOCK_SIZE, chunk=CHUNK):
    """what the engine does: plain components, and the chunked rule replayed on the members of the components of
    lock_size members or more alone.  Returns (labels, replayed k-mers)."""
    comp = components(keys, k)
    _, sizes = listing(comp)
    size_of = dict(zip(sorted(set(comp)), sizes))
    over = [i for i, l in enumerate(comp) if size_of[l] >= lock_size]
    lab = list(comp)
    for g, l in cluster(keys, k, lock_size, chunk, subset=over).items():
        lab[g] = l
    return lab, len(over)


def file_bytes(labels):
    """(kmers.hamming, kmers.hamming.idx)"""
    members, sizes = listing(labels)
    return np.array(members, dtype=np.uint64).tobytes(), np.array(sizes, dtype=np.uint64).tobytes()
