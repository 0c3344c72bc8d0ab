"""GPU: BayesHammer's stages over a set that Counter.finish(min_count=2) filtered (count_filter_singletons 1, DESIGN.md
4.3k), through the binding: the statistics, the expander's rounds and the corrected reads against the restatements over the
same smaller set.  The reads hold k-mers that the set does not: every stage meets its "not found" path."""
import pytest

import spades_for_blackbird_amd as B
from tests import expander_restated as E
from tests import hammer_filtered_case as Fc
from tests import kmerdata_restated as KR
from tests import readcorrect_restated as R
from tests import readprint_restated as P
from tests.hreads_child import arrays
from tests.test_gpu_kmerdata import _as_tuples, _check, _stretches, _upload

pytestmark = pytest.mark.gpu

K = Fc.K
NO_LIMIT = 1000


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case():
    g, recs = Fc.filtered_case()
    kmers, keys = Fc.filtered_set(recs)
    return g, recs, kmers, keys


@pytest.fixture(scope="module")
def filtered(ctx, case):
    """the filtered set of the reads' stretches, as pass 1 of spades-kmerdata --filter-singletons builds it"""
    _, recs, _, _ = case
    reads = [(s, q) for _, s, q in recs]
    rd, qu = _upload(ctx, _stretches(reads, K))
    c = ctx.counter(K, B.BOTH_STRANDS | B.WITH_COUNTS)
    c.push(rd)
    s = c.finish(min_count=2)
    yield s, rd, qu
    for x in (qu, rd, s):
        x.free()


def test_the_filter_drops_kmers_the_reads_hold(case, filtered):
    _, recs, kmers, keys = case
    s, _, _ = filtered
    counts = Fc.counted(recs)
    singletons = [km for km, c in counts.items() if c == 1]
    assert s.n_dropped == len(singletons) > 0 and len(kmers) > 0
    got, cnt = s.export(with_counts=True)
    assert [int(x) for x in got[:, 0]] == keys
    assert cnt.tolist() == [counts[km] for km in kmers] and int(cnt.min()) >= 2
    # the two lonely reads hold singletons only; a substituted base makes K singletons on either strand
    for name, seq, _ in recs:
        held = [seq[p:p + K] in counts and counts[seq[p:p + K]] >= 2 for p in range(len(seq) - K + 1)]
        assert any(held) != name.startswith("lonely"), name
    assert sum(1 for _, seq, _ in recs if not all(counts[seq[p:p + K]] >= 2 for p in range(len(seq) - K + 1))) >= 7


def test_statistics_over_the_filtered_set(case, filtered):
    _, recs, kmers, keys = case
    s, rd, qu = filtered
    ks = s.kmer_stats()
    assert len(ks) == len(keys)
    ks.push(rd, qu)
    ks.finish()
    exp = KR.fill_kmer_data([(sq, q) for _, sq, q in recs], K, kmer_set=set(kmers))
    assert set(exp) == set(kmers)
    _check(keys, K, ks.export(), _as_tuples(exp))
    ks.free()


def _good_at_first(g, kmers):
    """every third k-mer of the genome that the set holds, with its reverse complement"""
    start = set(R.kmers_of(g, K)[::3])
    start |= {KR.revcomp(x) for x in start}
    return [1 if km in start else 0 for km in kmers]


def test_expander_rounds_over_the_filtered_set(ctx, case, filtered):
    g, recs, kmers, _ = case
    s, _, _ = filtered
    index = {km: i for i, km in enumerate(kmers)}
    good = _good_at_first(g, kmers)
    cands = E.candidate_reads([(sq, q) for _, sq, q in recs], K)
    assert len(cands) == len(recs)
    closure, counts, states = E.snapshot_rounds(cands, K, index, good, None, 1)
    statuses = E.snapshot_round(cands, K, index, good)[2]
    assert 0 in statuses and 1 in statuses and len(counts) >= 2 and sum(closure) > sum(good) > 0
    assert any(index.get(c[p:p + K], -1) == -1 for c in cands for p in range(len(c) - K + 1))
    e = s.expander(good)
    rd = ctx.reads_from_ascii(cands)
    assert e.run(rd, max_rounds=NO_LIMIT, min_changed=1) == counts
    assert e.export().tolist() == closure
    e.free()
    rd.free()


def test_corrected_reads_over_the_filtered_set(ctx, case, filtered):
    g, recs, kmers, keys = case
    s, _, _ = filtered
    index = {km: i for i, km in enumerate(kmers)}
    cands = E.candidate_reads([(sq, q) for _, sq, q in recs], K)
    closure, _, _ = E.snapshot_rounds(cands, K, index, _good_at_first(g, kmers), None, 1)
    # the set as make_index states it: the expanded good k-mers (it marks their reverse complements too) and the others
    index2, keys2, good2 = R.make_index([km for km, b in zip(kmers, closure) if b], [km for km, b in zip(kmers, closure) if not b])
    assert (index2, keys2) == (index, keys) and sum(good2) >= sum(closure) and 0 in good2
    rc = R.ReadCorrector(index2, good2, K)
    rows = P.corrected_records(rc, recs, 4, True, 33)
    want = [x.encode("latin-1") for x in P.route_single(rows)]
    c = s.corrector(good2)
    hr = ctx.hammer_reads(*arrays([(sq, q) for _, sq, q in recs]), K)
    cr = c.correct_resident(hr)
    text = cr.print([n for n, _, _ in recs], tags=True)
    assert [text.stream(0), text.stream(1)] == want
    assert [c.stats[x] for x in B.Corrector.STATS[:4]] == rc.stats()
    kinds = {x[2] for x in rows}
    assert P.CHANGED in kinds and P.NONE in kinds, kinds  # a substitution is corrected; a lonely read finds no k-mer
    for x in (text, cr, hr, c):
        x.free()
