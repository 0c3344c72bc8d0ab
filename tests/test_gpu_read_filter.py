"""GPU: the per-read median multiplicity test (k_median_filter in csrc/readfilter.hip) on a crafted counted set, against a
direct evaluation of the median.  The set is built with kmerset_from_device from the reads' own canonical k-mers with
counts of the test's choosing: ties at the median, k-mers left out of the set (multiplicity 0), counts of 2^31 and above.
Every read is asked at 0, just below, at and just above its own median and at 0xFFFFFFFF; it must flip from kept to
dropped exactly above its median."""
import numpy as np
import pytest

import spades_for_blackbird_amd as B
from tests import kmerprofile_restated as R

pytestmark = pytest.mark.gpu

NKS = (1, 2, 3, 63, 64, 65, 128, 129)
U32 = 0xFFFFFFFF
# few distinct values: the median of most reads sits inside a run of equal multiplicities
POOL = (1, 2, 2, 3, 3, 3, 7, 255, 256, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, U32 - 1, U32)


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def torch_device():
    """torch's first use of the device, outside the timed cases"""
    import torch
    torch.zeros(1).cuda()
    torch.cuda.synchronize()


def _genome(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _case(k, seed=0):
    """(reads, {canonical k-mer: count}): per nk three reads -- most k-mers counted, most k-mers left out (median 0), all
    counts 2^31 or above -- plus the reverse complement of one read, an empty read and one of k - 1 bases"""
    rng = np.random.default_rng([k, seed])
    reads, counts = [], {}
    for nk in NKS:
        for kind in range(3):
            read = _genome(rng, nk + k - 1)
            reads.append(read)
            for j in range(nk):
                c = R.canonical(read[j:j + k])
                assert c not in counts and R.rc(c) != c
                if rng.random() < (0.2, 0.7, 0.0)[kind]:
                    continue  # not in the set: multiplicity 0
                counts[c] = int(POOL[int(rng.integers(0, len(POOL)))]) if kind < 2 else int(rng.integers(2 ** 31, U32 + 1))
    reads.append(R.rc(reads[3 * NKS.index(65)]))
    top = _genome(rng, 3 + k - 1)  # a median of 0xFFFFFFFF: no threshold drops it
    for j in range(3):
        counts[R.canonical(top[j:j + k])] = U32
    reads += [top, "", _genome(rng, k - 1)]
    return reads, counts


def _medians(reads, counts, k):
    out = []
    for read in reads:
        nk = len(read) - k + 1
        if nk < 1:
            out.append(0)  # CountMedianMlt of a read shorter than k
            continue
        m = sorted(counts.get(R.canonical(read[j:j + k]), 0) for j in range(nk))
        out.append(m[nk // 2])
    return out


def _device_set(ctx, k, counts, rng):
    import torch
    nw = R.words(k)
    recs = sorted((R.encode(km), c) for km, c in counts.items())
    keys = np.array([r[0] for r in recs], dtype=np.uint64).reshape(len(recs), nw)
    vals = np.array([r[1] for r in recs], dtype=np.uint32)
    order = rng.permutation(len(recs))
    dk = torch.from_numpy(np.ascontiguousarray(keys[order]).view(np.int64)).cuda()
    dc = torch.from_numpy(np.ascontiguousarray(vals[order]).view(np.int32)).cuda()
    torch.cuda.synchronize()
    s = ctx.kmerset_from_device(dk, len(recs), k, d_counts=dc, flags=B.CANONICAL)
    assert len(s) == len(recs)
    if recs:
        got_k, got_c = s.export(with_counts=True)
        assert got_k.tobytes() == keys.tobytes() and got_c.astype(np.uint32).tobytes() == vals.tobytes()
    return s


def _check(ctx, k, reads, counts):
    med = _medians(reads, counts, k)
    s = _device_set(ctx, k, counts, np.random.default_rng(k))
    rd = ctx.reads_from_ascii(reads)
    thresholds = sorted({0, U32} | {t for m in med for t in (m - 1, m, m + 1) if 0 <= t <= U32})
    keep = {t: ctx.median_filter(rd, s, t).tolist() for t in thresholds}
    for t in thresholds:
        assert keep[t] == [int(m >= t) for m in med], (k, t)
    for i, m in enumerate(med):  # kept up to its own median, dropped right above it
        assert keep[m][i] == 1 and keep[0][i] == 1
        if m < U32:
            assert keep[m + 1][i] == 0
    return med, keep


@pytest.mark.parametrize("k", [21, 31, 33, 63, 65, 97, 127])
def test_median_filter_on_crafted_counts(ctx, k):
    reads, counts = _case(k)
    med, keep = _check(ctx, k, reads, counts)
    assert [len(r) - k + 1 for r in reads[:3 * len(NKS)]] == [nk for nk in NKS for _ in range(3)]
    assert med.count(0) >= 7 and sum(1 for m in med if m >= 2 ** 31) >= len(NKS) and U32 in med
    assert med[-4] == med[3 * NKS.index(65)]  # a read and its reverse complement
    assert sum(keep[U32]) == med.count(U32) >= 1
    # an empty read and a read shorter than k are kept at threshold 0 only
    assert [keep[t][-2:] for t in (0, 1, U32)] == [[1, 1], [0, 0], [0, 0]]
    # reads whose median sits inside a run of equal multiplicities, and reads where it is the last of its run
    inside = 0
    for read, m in zip(reads[:3 * len(NKS)], med):
        nk = len(read) - k + 1
        ms = sorted(counts.get(R.canonical(read[j:j + k]), 0) for j in range(nk))
        inside += nk > 2 and ms[nk // 2 - 1] == m
    assert inside >= 6


@pytest.mark.parametrize("k", [21, 33, 65, 127])
def test_median_filter_with_wide_index_entries(ctx, monkeypatch, k):
    reads, counts = _case(k, seed=1)
    med, keep = _check(ctx, k, reads, counts)
    monkeypatch.setenv("BBK_WIDE_INDEX", "1")
    assert _check(ctx, k, reads, counts) == (med, keep)


def test_median_filter_with_an_empty_set(ctx):
    """no k-mer at all: every multiplicity is 0 and every read is kept at threshold 0 only"""
    import torch
    k = 33
    reads, _ = _case(k)
    # no record: the arrays are not read, but a set with counts needs a counts pointer
    empty = ctx.kmerset_from_device(torch.zeros(2, dtype=torch.int64).cuda(), 0, k,
                                    d_counts=torch.zeros(1, dtype=torch.int32).cuda(), flags=B.CANONICAL)
    assert len(empty) == 0
    rd = ctx.reads_from_ascii(reads)
    assert ctx.median_filter(rd, empty, 0).tolist() == [1] * len(reads)
    for t in (1, 2 ** 31, U32):
        assert ctx.median_filter(rd, empty, t).tolist() == [0] * len(reads)
