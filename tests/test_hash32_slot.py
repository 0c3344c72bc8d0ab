"""CPU: the table slot of stage A's narrow dedup kernel (k_bucket_hash32, msd_narrow_a.h: nw_hslot).

The kernel puts the 4-byte record lo of a bucket into an LDS table of 8192 slots by linear probing.  Until round 11 the
slot was nw_slot(nw_mix(lo)) -- a third multiply on top of the two of the mix; now it is the top 13 bits of the mix's
FIRST product, (lo * 0x9E3779B1) >> 19.  Segment and level-2 bin fix bits of nw_mix(lo) inside a bucket, so the new
slot must be shown to spread the keys of a bucket as well as the old one did.

Input: the canonical 21-mers of a uniform genome and of an AT-rich genome full of noisy tandem repeats (seeded, 1.5 M
bases each), restated here in numpy and grouped into the 1024 level-1 segments the kernels group them into (nw_bin1;
one bucket per segment, as a call of this size is planned).  Measure: mean extra probes per distinct key when the keys
of every bucket are inserted by linear probing.  The old function is the reference: the new one may need at most
1.10 x its mean + 0.01 per key (the two differ by about +-1 % on these inputs: 0.1091 / 0.1091 and 0.0815 / 0.0814
when the issue was written).
"""
import numpy as np
import pytest

K = 21
SLOTS = 8192
M32 = np.uint64(0xFFFFFFFF)


def nw_mix(lo):
    t = (lo * np.uint64(0x9E3779B1)) & M32
    t ^= t >> np.uint64(15)
    t = (t * np.uint64(0x85EBCA6B)) & M32
    t ^= t >> np.uint64(13)
    return t


def slot_old(lo):
    return ((nw_mix(lo) * np.uint64(0x27D4EB2F)) & M32) >> np.uint64(19)


def slot_new(lo):
    return ((lo * np.uint64(0x9E3779B1)) & M32) >> np.uint64(19)


def canonical_kmers(bases, k):
    """distinct canonical k-mers of a base array (values 0..3), base i of a k-mer in bits 2i .. 2i+1; the canonical
    one of a k-mer and its reverse complement is the smaller in base order (first base most significant)"""
    n = len(bases) - k + 1
    b = bases.astype(np.uint64)
    fwd = np.zeros(n, np.uint64)   # k-mer, base i at bits 2i
    rev = np.zeros(n, np.uint64)   # reverse complement, laid out the same way
    fwd_m = np.zeros(n, np.uint64)  # the same two with the first base most significant
    rev_m = np.zeros(n, np.uint64)
    for i in range(k):
        f = b[i:i + n]
        r = np.uint64(3) - b[k - 1 - i:k - 1 - i + n]
        fwd |= f << np.uint64(2 * i)
        rev |= r << np.uint64(2 * i)
        fwd_m |= f << np.uint64(2 * (k - 1 - i))
        rev_m |= r << np.uint64(2 * (k - 1 - i))
    return np.unique(np.where(fwd_m <= rev_m, fwd, rev))


def uniform_genome(n, seed):
    return np.random.default_rng(seed).integers(0, 4, size=n, dtype=np.uint8)


def low_complexity_genome(n, seed):
    """AT-rich stretches (A, T 40 % each) between tandem repeats of a 2..12-base unit, 5..40 copies, 2 % of their
    bases replaced"""
    rng = np.random.default_rng(seed)
    parts, have = [], 0
    while have < n:
        bg = rng.choice(4, size=int(rng.integers(20, 200)), p=[0.4, 0.1, 0.1, 0.4]).astype(np.uint8)
        unit = rng.choice(4, size=int(rng.integers(2, 13)), p=[0.4, 0.1, 0.1, 0.4]).astype(np.uint8)
        rep = np.tile(unit, int(rng.integers(5, 41)))
        noisy = rng.random(len(rep)) < 0.02
        rep[noisy] = rng.integers(0, 4, size=int(noisy.sum()), dtype=np.uint8)
        parts += [bg, rep]
        have += len(bg) + len(rep)
    return np.concatenate(parts)[:n]


def buckets_of(keys, k):
    """level-1 segment of every key (nw_bin1) and its 4-byte record"""
    hb = 2 * k - 32
    lo, hi = keys & M32, keys >> np.uint64(32)
    seg = (nw_mix(lo) >> np.uint64(22)) ^ (hi << np.uint64(10 - hb))
    return seg.astype(np.int64), lo


def extra_probes(bucket, slot):
    """Total extra probes of linear probing into SLOTS slots per bucket.  All keys advance together: in every round a
    waiting key tries its next slot, one key per free (bucket, slot) takes it.  A key only ever passes slots that were
    taken when it tried them, so this is a linear-probing run in some insertion order -- and the total does not depend
    on the order."""
    taken = np.zeros(int(bucket.max() + 1) * SLOTS, bool)
    at = bucket * SLOTS + slot.astype(np.int64)
    base = bucket * SLOTS
    total = 0
    while len(at):
        free = ~taken[at]
        _, first = np.unique(at[free], return_index=True)
        win = np.flatnonzero(free)[first]
        taken[at[win]] = True
        keep = np.ones(len(at), bool)
        keep[win] = False
        at, base = at[keep], base[keep]
        total += len(at)
        at = base + (at - base + 1) % SLOTS
    return total


@pytest.mark.parametrize("name,genome", [("uniform", uniform_genome), ("low-complexity", low_complexity_genome)])
def test_new_slot_probes_like_the_old_one(name, genome):
    keys = canonical_kmers(genome(1_500_000, 20261019), K)
    bucket, lo = buckets_of(keys, K)
    assert bucket.min() >= 0 and bucket.max() < 1024
    old = extra_probes(bucket, slot_old(lo)) / len(keys)
    new = extra_probes(bucket, slot_new(lo)) / len(keys)
    print("%s: %d keys, mean extra probes per key old %.4f new %.4f" % (name, len(keys), old, new))
    assert new <= 1.10 * old + 0.01, (name, old, new)
