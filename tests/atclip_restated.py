"""Sequential, in-place restatement of EarlyLowComplexityClipperProcessor (the reference's
assembly_graph/construction/early_simplification.hpp:163-344): RemoveATEdges and RemoveATTips as one thread runs them,
changing the masks while it walks.  The parity target of csrc/atclip.hip, which collects against a snapshot instead.

An Index holds (canonical k-mer string -> InOutMask byte): bits 0-3 outgoing A,C,G,T, bits 4-7 incoming, stored for
the canonical form; the other orientation reads the bit-reversed byte (InOutMask::conjugate)."""
import struct

import numpy as np

ACGT = "ACGT"
IDX = {c: i for i, c in enumerate(ACGT)}
_COMP = str.maketrans("ACGT", "TGCA")
_POP = [bin(i).count("1") for i in range(16)]


def rc(s):
    return s[::-1].translate(_COMP)


def rev8(m):
    return int("{:08b}".format(m)[::-1], 2)


def _biased(v):
    s = struct.unpack("<Q", struct.pack("<d", v))[0]
    return ((~s + 1) & 0xFFFFFFFFFFFFFFFF) if s >> 63 else s | (1 << 63)


def ls(a, b):
    """math::ls (math/xmath.h:218-226,251-268,300-305): a < b, unless a and b lie within 4 ULPs of each other."""
    return abs(_biased(float(a)) - _biased(float(b))) > 4 and a < b


def junction(m):
    return _POP[m & 15] != 1 or _POP[m >> 4] != 1


def kmer_strings(keys, k):
    """(n, words) uint64 key records (base i in bits 2(i%32).. of word i/32) -> list of k-mer strings"""
    keys = np.asarray(keys, dtype=np.uint64)
    if len(keys) == 0:
        return []
    pos = np.arange(k)
    bases = (keys[:, pos >> 5] >> ((pos & 31) * 2).astype(np.uint64)) & np.uint64(3)
    txt = np.frombuffer(b"ACGT", dtype=np.uint8)[bases.astype(np.intp)]
    return [b.decode() for b in np.ascontiguousarray(txt).view("S%d" % k).ravel()]


class Index:
    """DeBruijnExtensionIndex on a dict: the oriented accessors the two passes use."""

    def __init__(self, kmers, masks, k):
        self.k = k
        self.kmers = list(kmers)
        self.masks = [int(m) for m in masks]
        self.pos = {s: i for i, s in enumerate(self.kmers)}

    @classmethod
    def from_oracle(cls, ox):
        return cls(kmer_strings(ox.kmers, ox.k), ox.masks, ox.k)

    def _locate(self, s):
        i = self.pos.get(s)
        return (i, False) if i is not None else (self.pos[rc(s)], True)

    def get(self, s):
        i, flip = self._locate(s)
        return rev8(self.masks[i]) if flip else self.masks[i]

    def set(self, s, m):
        i, flip = self._locate(s)
        self.masks[i] = rev8(m) if flip else m

    def delete_outgoing(self, s, c):
        self.set(s, self.get(s) & ~(1 << c))

    def delete_incoming(self, s, c):
        self.set(s, self.get(s) & ~(1 << (4 + c)))

    def mask_array(self):
        return np.array(self.masks, dtype=np.uint8)

    def oriented(self):
        """every stored k-mer in both orientations, in storage order (the reference's `for s : {seq, !seq}`)"""
        for s in self.kmers:
            yield s
            yield rc(s)


def remove_at_edges(ix, ratio):
    """RemoveATEdges (:183-257): returns (collected edges, removed links)."""
    thr = ix.k * ratio
    edges = []
    for s in ix.oriented():
        m = ix.get(s)
        if not junction(m):
            continue
        if ls(max(s.count(c) for c in ACGT), thr):
            continue
        for c in range(4):
            if m >> c & 1 and junction(ix.get(s[1:] + ACGT[c])):  # IsJunction || IsDeadEnd
                edges.append((s, c))
    links = 0
    for s, c in edges:
        if not ix.get(s) >> c & 1:
            continue
        ix.delete_outgoing(s, c)
        ix.delete_incoming(s[1:] + ACGT[c], IDX[s[0]])
        links += 2
    return len(edges), links


def remove_inconsistent_forward_links(ix, x):
    """RemoveInconsistentForwardLinks (:20-35)"""
    count = 0
    m = ix.get(x)
    for c in range(4):
        if m >> c & 1 and not ix.get(x[1:] + ACGT[c]) >> (4 + IDX[x[0]]) & 1:
            ix.delete_outgoing(x, c)
            count += 1
    return count


def remove_at_tips(ix, ratio, min_len, max_len):
    """RemoveATTips (:269-333): returns (isolated k-mers, clipped links)."""
    k = ix.k
    removed = 0
    junctions = []
    for s in ix.oriented():
        m = ix.get(s)
        if m & 15 or _POP[m >> 4] != 1:  # !IsDeadEnd || !CheckUniqueIncoming
            continue
        tip, counts, x = [], [0, 0, 0, 0], s
        while True:
            tip.append(x)
            counts[IDX[x[k - 1]]] += 1
            x = ACGT[(ix.get(x) >> 4).bit_length() - 1] + x[:-1]  # GetUniqueIncoming
            if not (len(tip) < max_len and not junction(ix.get(x))):
                break
        xm = ix.get(x)
        if xm >> 4 == 0 or not junction(xm):  # IsDeadStart || !IsJunction
            continue
        for i in range(len(tip) - 1, min_len):
            counts[IDX[x[k - 1 - i]]] += 1
        if ls(max(counts), max(len(tip), min_len) * ratio):
            continue
        junctions.append(x)
        removed += len(tip)
        for t in tip:
            ix.set(t, 0)  # IsolateVertex
    links = sum(remove_inconsistent_forward_links(ix, x) for x in junctions)
    return removed, links
