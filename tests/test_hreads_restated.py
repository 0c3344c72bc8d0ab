"""The closed form of the trim and of the valid-k-mer generator (tests/hreads_restated.py: what k_hr_prepare implements)
against the literal rules of tests/kmerdata_restated.py, for both nucleotide predicates.  No GPU."""
import numpy as np
import pytest

from tests import hreads_restated as HR
from tests import kmerdata_restated as KR
from tests import readcorrect_restated as RR


def _compare(records, k, tq):
    for seq, qual in records:
        t = HR.closed_trim(seq, qual, tq)
        assert t == HR.literal_trim(seq, qual, tq), (seq, qual)
        s, q, ltrim_, rtrim_, initial = RR.trim_read(seq, qual, tq)  # the bookkeeping of Read::print follows from t
        assert (ltrim_, rtrim_) == ((t[0], t[0] + t[1]) if t[1] else (0, initial)) and len(s) == t[1], (seq, qual)
        s, q = seq[t[0]:t[0] + t[1]], list(qual[t[0]:t[0] + t[1]])
        for name, pred in HR.PREDICATES.items():
            assert HR.closed_starts(s, q, k, pred) == HR.literal_starts(s, q, k, pred), (name, seq, qual)
        if t[1] >= k:  # the file's own generator, which runs behind the trim (KMerDataFiller)
            assert [x + t[0] for x in HR.closed_starts(s, q, k, HR.is_nucl_kmer)] == KR.valid_starts(seq, qual, k, tq), (seq, qual)
        else:
            assert KR.valid_starts(seq, qual, k, tq) == []


@pytest.mark.parametrize("k", [5, 21, 32])
def test_closed_form_on_crafted_reads(k):
    rng = np.random.default_rng(100 + k)
    recs = [(s, q) for _, s, q in KR.crafted_reads(k, rng)]
    recs += [(s.lower(), q) for s, q in recs[:6]] + [(s.replace("N", "."), q) for s, q in recs[4:8]]
    _compare(recs, k, 4)


@pytest.mark.parametrize("k", [3, 5, 21, 31])
def test_closed_form_on_random_reads(k):
    rng = np.random.default_rng(7 * k)
    recs = HR.random_records(rng, 1500, k=k)
    _compare(recs, k, 4)
    _compare(recs[:300], k, 0)
    _compare(recs[:300], k, 1)


def test_prepare_closed_equals_prepare():
    rng = np.random.default_rng(3)
    recs = [("", [])] + HR.random_records(rng, 400, k=5) + [("", [])]
    assert HR.prepare_closed(recs, 5, 4) == HR.prepare(recs, 5, 4)
    got = HR.prepare(recs, 5, 4)
    assert any(got[3]) and not all(got[3]) and any(len(x) > 1 for x in got[1])


def test_candidates_are_the_expander_restatement():
    from tests import expander_restated as ER
    rng = np.random.default_rng(11)
    recs = HR.random_records(rng, 300, k=5, odd=0.03)
    trims, _, _, cand = HR.prepare(recs, 5, 4)
    want = ER.candidate_reads(recs, 5)
    assert 10 < len(want) < len(recs)
    assert [recs[i][0][t[0]:t[0] + t[1]].upper() for i, t in enumerate(trims) if cand[i]] == want


@pytest.mark.parametrize("k", [5, 21, 32])
def test_identity_trim_closed_form(k):
    """a batch that is trimmed already (BBK_NO_TRIM): the closed-form starts over whole records equal the literal ones,
    bad ends, Ns and all"""
    rng = np.random.default_rng(40 + k)
    recs = [("", [])] + HR.random_records(rng, 600, k=k) + HR.boundary_records(np.random.default_rng(9))
    got = HR.prepare(recs, k, None, trim=HR.identity_trim, starts=HR.closed_starts)
    assert got == HR.prepare(recs, k, None, trim=HR.identity_trim)
    assert got[0] == [(0, len(s)) for s, _ in recs]
    assert any(got[3]) and not all(got[3]) and any(len(x) > 1 for x in got[2])
