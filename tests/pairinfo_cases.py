"""Inputs of the paired-info tests (pure Python): the genome of Context.reads_synth restated, read pairs cut from a
genome, and the run of one library through the restatement and through the engine."""
import random

import numpy as np

from tests import pairinfo_restated as P
from tests.helpers import rc

_M = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M
    return x ^ (x >> 31)


def synth_genome(seed_genome, n):
    """the genome bbk_reads_synth draws its reads from: base g is 2 bits of splitmix64(seed_genome + g / 32)"""
    out = []
    for w in range((n + 31) // 32):
        v = _splitmix64(seed_genome + w)
        out.append("".join("ACGT"[(v >> (2 * j)) & 3] for j in range(32)))
    return "".join(out)[:n]


def mutate(rng, s, sub=0.01, n=0.004):
    """_mutate of tests/test_gpu_gmapper.py"""
    out = []
    for c in s:
        x = rng.random()
        out.append("N" if x < n else rng.choice("ACGT".replace(c, "")) if x < n + sub else c)
    return "".join(out)


def cut_pairs(rng, genome, n, read_len=150, mean=400, sd=30):
    """n pairs of an fr library: fragments of length ~ N(mean, sd), either strand.  Every fourth pair has its second
    mate on the other strand (so fr presents it on the conjugate edge), every sixteenth is an outie (rf in the file:
    a negative insert size under fr)"""
    pairs = []
    for i in range(n):
        F = max(read_len, int(round(rng.gauss(mean, sd))))
        a = rng.randint(0, len(genome) - F)
        frag = genome[a:a + F]
        if rng.random() < 0.5:
            frag = rc(frag)
        first, second = frag[:read_len], rc(frag[-read_len:])
        if i % 16 == 7:
            first, second = rc(first), rc(second)
        elif i % 4 == 3:
            second = rc(second)
        pairs.append((first, second))
    return pairs


def cuts(pairs):
    """np.uint32 [n, 4]: left1, right1, left2, right2 of LongestValid, in file orientation"""
    out = np.zeros((len(pairs), 4), dtype=np.uint32)
    for i, (a, b) in enumerate(pairs):
        (_, out[i, 0], out[i, 1]), (_, out[i, 2], out[i, 3]) = P.longest_valid(a), P.longest_valid(b)
    return out


def restated(g, pairs, orientation, min_edge_length=0, round_distance=0, threshold=0, insert_size=None):
    """(statistics, histogram, points, library) of the restatement; insert_size None: (size_t) mean, as the reference"""
    lib = P.Library(g, min_edge_length)
    lib.push_estimate(pairs, orientation)
    st = lib.estimate()
    if insert_size is None:
        insert_size = int(st["mean"])
    lib.push_fill(pairs, orientation, insert_size, round_distance, threshold)
    return st, lib.hist(), lib.points(), lib


def engine(ctx, ix, pairs, orientation, min_edge_length=0, round_distance=0, threshold=0, insert_size=None, batches=None,
           with_cut=True, prd=None):
    """(statistics, histogram, points) of the engine; batches: the sizes the pairs are pushed in (one batch if None)"""
    batches = [len(pairs)] if batches is None else batches
    assert sum(batches) == len(pairs)
    pi = ix.pairinfo(min_edge_length)
    parts, at = [], 0
    for n in batches:
        part = pairs[at:at + n]
        at += n
        parts.append((ctx.reads_from_ascii([a for a, _ in part]), ctx.reads_from_ascii([b for _, b in part]),
                      cuts(part) if with_cut else None))
    for first, second, cut in parts:
        pi.push_estimate(first, second, orientation, cut)
    st = pi.estimate()
    his, cnt = pi.hist()
    pi.fill_begin(int(st["mean"]) if insert_size is None else insert_size, round_distance, threshold)
    for first, second, cut in parts:
        pi.push_fill(first, second, orientation, cut)
    pi.fill_finish()
    e1, e2, gap, w = pi.points()
    if prd is not None:
        pi.write(prd)
    return (st, list(zip(his.tolist(), cnt.tolist())), list(zip(e1.tolist(), e2.tolist(), gap.tolist(), w.tolist())))
