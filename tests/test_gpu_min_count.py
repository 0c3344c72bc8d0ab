"""GPU: Counter.finish(min_count) (bbk_count_finish_min_count) against numpy on the unfiltered result of
the same reads and flags -- keys, counts, stored order and n_dropped -- at set sizes around the tile of the selection, with
kept and dropped records alternating, for every key width and every order flag.  Bit-exact: integer work."""
import numpy as np
import pytest

import spades_for_blackbird_amd as B
from tests.helpers import rc

pytestmark = pytest.mark.gpu

T = 256  # the tile of the ordered selection (select.h: kSelTile): distinct canonical records, the filter's input
SIZES = (0, 1, T - 1, T, T + 1, 3 * T + 5)
MIN_COUNTS = (0, 1, 2, 3, 2 ** 32 - 1)
FLAGS = {"both": B.BOTH_STRANDS, "canonical": B.CANONICAL, "both_ref": B.BOTH_STRANDS | B.REFERENCE_ORDER}


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def crafted_reads(k, n, seed, twice="alternate"):
    """One read with exactly n distinct canonical k-mers, none its own reverse complement, and short reads that repeat
    every second of them (twice="alternate"), all of them ("all") or none ("none")"""
    if n == 0:
        return ["ACGT"[:min(4, k - 1)]]  # a read too short for a k-mer
    rng = np.random.default_rng(seed)
    while True:
        s = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n + k - 1)]).decode()
        kmers = [s[i:i + k] for i in range(n)]
        if len({min(x, rc(x)) for x in kmers}) == n and all(x != rc(x) for x in kmers):
            break
    step = {"alternate": 2, "all": 1}.get(twice)
    return [s] + (kmers[::step] if step else [])


def finish(ctx, batches, k, flags, min_count=None):
    c = ctx.counter(k, flags | B.WITH_COUNTS)
    for reads in batches:
        c.push(ctx.reads_from_ascii(reads))
    s = c.finish() if min_count is None else c.finish(min_count=min_count)
    keys, cnt = s.get(0, len(s), with_counts=True)  # the records as they are stored
    return s, keys, cnt


def check_filtered(ctx, batches, k, flags, min_counts=MIN_COUNTS):
    _, keys, cnt = finish(ctx, batches, k, flags)
    for mc in min_counts:
        s, fk, fc = finish(ctx, batches, k, flags, mc)
        keep = cnt.astype(np.uint64) >= np.uint64(mc)  # (every count is at least 1: 0 and 1 keep everything)
        assert fk.tobytes() == keys[keep].tobytes(), (k, flags, mc)
        assert fc.tobytes() == cnt[keep].tobytes(), (k, flags, mc)
        assert s.n_dropped == int((~keep).sum()), (k, flags, mc)
        assert s.device_keys()[1] == (B.ORDER_REFERENCE_BUCKETS16 if flags & B.REFERENCE_ORDER else B.ORDER_SORTED)
        if mc == 2 ** 32 - 1:
            assert len(s) == 0
    return keys, cnt


@pytest.mark.parametrize("flags", sorted(FLAGS))
@pytest.mark.parametrize("k", [21, 33, 97])  # W = 1, 2 and 4
def test_sizes_around_the_tile(ctx, k, flags):
    for n in SIZES:
        reads = crafted_reads(k, n, seed=1000 * k + n)
        keys, cnt = check_filtered(ctx, [reads], k, FLAGS[flags])
        per = 1 if flags == "canonical" else 2
        assert len(keys) == per * n
        assert (int((cnt == 2).sum()), int((cnt == 1).sum())) == (per * ((n + 1) // 2), per * (n // 2))  # they alternate


@pytest.mark.parametrize("flags", sorted(FLAGS))
def test_all_kept_and_all_dropped(ctx, flags):
    k, n = 21, 3 * T + 5
    for twice, kept_at_2 in (("all", True), ("none", False)):
        reads = crafted_reads(k, n, seed=7, twice=twice)
        s, _, _ = finish(ctx, [reads], k, FLAGS[flags], 2)
        total = n if flags == "canonical" else 2 * n
        assert (len(s), s.n_dropped) == ((total, 0) if kept_at_2 else (0, total))
        check_filtered(ctx, [reads], k, FLAGS[flags], (2, 3))


def test_self_complement_counts_twice(ctx):
    """k = 4: ACGT is its own reverse complement, so its one occurrence is exported with multiplicity 2 by a both-strand
    set and survives min_count = 2; CGTT next to it (canonical AACG) occurs once and does not"""
    reads = ["ACGTT"]
    for name in ("both", "both_ref"):
        keys, cnt = check_filtered(ctx, [reads], 4, FLAGS[name])
        assert sorted(cnt.tolist()) == [1, 1, 2]
        s, fk, fc = finish(ctx, [reads], 4, FLAGS[name], 2)
        assert fk.tolist() == keys[cnt == 2].tolist() and fc.tolist() == [2] and s.n_dropped == 2
    # the canonical set exports one occurrence as 1: both records go
    s, fk, _ = finish(ctx, [reads], 4, FLAGS["canonical"], 2)
    assert len(fk) == 0 and s.n_dropped == 2
    check_filtered(ctx, [reads], 4, FLAGS["canonical"])
    # more self-complementary k-mers, among kept and dropped ones
    more = ["ACGTACGTAATTGGCC", "AATT", "TTAACCGGT", "GATCGATC", "CATGA"]
    for name in FLAGS:
        for k in (4, 6):
            check_filtered(ctx, [more], k, FLAGS[name], (2, 3, 4, 5))


@pytest.mark.parametrize("k", [21, 33])
def test_split_pushes_equal_one_push(ctx, k):
    reads = crafted_reads(k, 3 * T + 5, seed=k)
    half = len(reads) // 2
    for name in FLAGS:
        for mc in (2, 3):
            one, k1, c1 = finish(ctx, [reads], k, FLAGS[name], mc)
            two, k2, c2 = finish(ctx, [reads[:half], reads[half:]], k, FLAGS[name], mc)
            assert k1.tobytes() == k2.tobytes() and c1.tobytes() == c2.tobytes() and one.n_dropped == two.n_dropped
            assert one.n_dropped > 0 and (len(one) > 0) == (mc == 2)  # (the counts are 1 and 2)


def test_counter_without_counts_is_refused(ctx):
    reads = crafted_reads(21, 10, seed=3)
    c = ctx.counter(21, B.BOTH_STRANDS)
    c.push(ctx.reads_from_ascii(reads))
    with pytest.raises(B.BBKError, match=r"bbk error -1: .*BBK_WITH_COUNTS"):  # BBK_ERR_ARG
        c.finish(min_count=2)
    c = ctx.counter(21, B.CANONICAL | B.WITH_MASKS)
    with pytest.raises(B.BBKError, match=r"bbk error -1: "):
        c.finish(min_count=2)
    check_filtered(ctx, [reads], 21, B.BOTH_STRANDS, (2,))  # the context goes on
