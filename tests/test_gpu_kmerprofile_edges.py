"""GPU: the profile kernels on crafted tables (tests/kmerprofile_cases.py; tests/test_kmerprofile_cases.py shows on the
CPU that the cases hold the classes they claim and tell wrong selections apart).

Abundance (k_ab_collect<W>, k_ab_reduce<TWO>): profiles the test writes itself and loads with kmerprofile_load, in all
four key widths and at both sides of every word boundary; every integer equals the restatement.  Join
(the per-sample selection on counts >= ci, k_kp_scatter, k_kp_keep and the selection on its keep byte): samples made
with kmerset_from_device from counts at ci, cs and the 16- and 32-bit limits.  Both look keys up through table_find over a PrefixIndex: tables of 1, 2 and 129
keys, one whose keys share a single bin, and 64-bit table entries (BBK_WIDE_INDEX)."""
import os
import subprocess

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build, build_host
from tests import kmerprofile_cases as K
from tests import kmerprofile_restated as R
from tests.helpers import check_profile_join

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bins():
    build.build()
    return {os.path.basename(p): p for p in build_host.build()}


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch_device():
    """torch's first use of the device, outside the timed cases"""
    import torch
    torch.zeros(1).cuda()
    torch.cuda.synchronize()


# ---- abundance ----------------------------------------------------------------------------------------------------------

def _write(case, prefix):
    keys, rows, kb, bb = K.table_files(case)
    with open(prefix + ".kmers", "wb") as f:
        f.write(kb)
    with open(prefix + ".bpr", "wb") as f:
        f.write(bb)
    return keys, kb, bb


def _ints(result):
    n, pos, sm, sq = result
    return [(int(a), int(b), [int(x) for x in c], [int(x) for x in d]) for a, b, c, d in zip(n, pos, sm, sq)]


def _abundance(ctx, tmp_path, case, tag):
    """loads the case's table and requires n, positions, sum and sumsq of every contig to equal the restatement's, with
    the contigs as runs of pieces and, for those of one piece, as reads of their own"""
    prefix = str(tmp_path / tag)
    keys, kb, bb = _write(case, prefix)
    p = ctx.kmerprofile_load(prefix, case["k"], case["N"])
    assert len(p) == len(keys) and p.keys().tobytes() == kb and p.rows().tobytes() == bb
    exp = K.expected(case)
    pieces, first = K.pieces_of(case["contigs"])
    got = _ints(p.abundance(ctx.reads_from_ascii(pieces), first))
    for (name, _), g, e in zip(case["contigs"], got, exp):
        assert g == e, (tag, name)
    single = [i for i, (_, seq) in enumerate(case["contigs"]) if len(R.split_on_ns(seq)) == 1]
    if single:
        got1 = _ints(p.abundance(ctx.reads_from_ascii([R.split_on_ns(case["contigs"][i][1])[0] for i in single])))
        assert got1 == [exp[i] for i in single], tag
    return got


def _cases(k):
    """(tag, case): the 16-bit and the 8-bit profile (k_ab_reduce<true> / <false>), the clustered tables, tiny tables"""
    main = K.crafted(k)
    out = [("main", main), ("eight", K.crafted(k, eight=True)), ("cluster", K.clustered(k)),
           ("cluster8", K.clustered(k, eight=True))]
    return out + [("keys%d" % n, K.restricted(main, n)) for n in (1, 2, 129)]


@pytest.mark.parametrize("k", [21, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127])
def test_abundance_of_crafted_profiles(ctx, tmp_path, k):
    for tag, case in _cases(k):
        _abundance(ctx, tmp_path, case, tag)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_abundance_at_small_k(ctx, tmp_path, k):
    _abundance(ctx, tmp_path, K.small_k(k), "small")


@pytest.mark.parametrize("k", [31, 63, 95, 127])
def test_abundance_with_wide_index_entries(ctx, tmp_path, monkeypatch, k):
    """the prefix table of a loaded profile with u64 entries: the same integers"""
    narrow = {tag: _abundance(ctx, tmp_path, case, tag) for tag, case in _cases(k)}
    monkeypatch.setenv("BBK_WIDE_INDEX", "1")
    for tag, case in _cases(k):
        assert _abundance(ctx, tmp_path, case, tag + "_wide") == narrow[tag]


def test_contig_abundance_counter_on_the_crafted_profile(bins, tmp_path):
    """the tool's text: a line at a share of exactly 70/100, none at 69/100, variances next to 65535 squared"""
    k, case = 33, K.crafted(33)
    prefix = str(tmp_path / "crafted")
    _write(case, prefix)
    fa, out = tmp_path / "contigs.fasta", tmp_path / "ab.tsv"
    fa.write_text("".join(">%s\n%s\n" % c for c in case["contigs"]))
    r = subprocess.run([bins["contig_abundance_counter"], "-k", str(k), "-c", str(fa), "-n", "7", "-m", prefix, "-o", str(out),
                        "-v"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = R.run(case["contigs"], k, case["table"], 7, var=True)
    assert out.read_text() == text
    names = [line.split("\t")[0] for line in text.split("\n")[:-1]]
    assert "share70" in names and "n2" in names and "share69" not in names


# ---- join ---------------------------------------------------------------------------------------------------------------

N_JOIN = 4
MIN_MULT = 5


def _join_keys(rng, k, n):
    """n distinct k-mers that begin with A and end in A, C or G (their own canonical form); the first six are two
    families that differ in their last base only, which for k > 32 means in their last word only"""
    kms = []
    for _ in range(2):
        stem = "A" + "".join("ACGT"[i] for i in rng.integers(0, 4, k - 2))
        kms += [stem + b for b in "ACG"]
    while len(set(kms)) < n:
        kms.append("A" + "".join("ACGT"[i] for i in rng.integers(0, 4, k - 2)) + "ACG"[int(rng.integers(0, 3))])
    kms = list(dict.fromkeys(kms))[:n]
    assert all(R.canonical(km) == km for km in kms)
    return kms


def _join_samples(k, union, ci, cs, seed):
    """per sample {k-mer: count}.  Sample 2 is empty and every count of sample 3 lies below ci.  The counts of samples 0
    and 1 walk through the values around ci, cs, MIN_MULT and the 16- and 32-bit limits; chosen keys pin the keep rule.
    Exactly `union` k-mers reach ci in some sample: that many keys the union of the filtered samples holds."""
    rng = np.random.default_rng([k, union, ci, cs, seed])
    kms = _join_keys(rng, k, union + 64)
    values = [ci - 1, ci, ci + 1, cs - 1, cs, cs + 1, 65535, 65536, 2 ** 32 - 1, MIN_MULT, MIN_MULT + 1, MIN_MULT - 1]
    nv = len(values)
    s0, s1, s3 = {}, {}, {}
    for i, km in enumerate(kms[:6]):  # the families: in sample 0, in sample 1, in both
        if i % 3 != 1:
            s0[km] = values[(2 * i + 1) % nv]
        if i % 3 != 0:
            s1[km] = ci
    for km, v in zip(kms[6:6 + nv], values):  # one sample present: kept iff the filtered count exceeds min_mult
        s0[km] = v
    for i, (km, v) in enumerate(zip(kms[6 + nv:6 + 2 * nv], values)):  # two samples present: kept whatever the total
        s0[km] = v
        s1[km] = values[(i + 1) % nv]
    s0[kms[6 + 2 * nv]] = s1[kms[6 + 2 * nv]] = ci  # present twice at the smallest count there is

    def reach():
        return sum(1 for km in set(s0) | set(s1) if max(s0.get(km, 0), s1.get(km, 0)) >= ci)
    for km in kms[7 + 2 * nv:]:
        if reach() == union:
            break
        which = int(rng.integers(0, 3))
        if which != 1:
            s0[km] = values[int(rng.integers(0, nv))]
        if which != 0:
            s1[km] = values[int(rng.integers(0, nv))]
    assert reach() == union
    for km in sorted(set(s0) | set(s1))[::3]:
        s3[km] = int(rng.integers(0, ci))
    return [s0, s1, {}, s3]


def _device_set(ctx, k, sample, rng):
    """the counted canonical set of one sample, from its records in random order; also (keys, counts) ascending"""
    import torch
    nw = R.words(k)
    recs = sorted((R.encode(km), c) for km, c in sample.items())
    keys = np.array([r[0] for r in recs], dtype=np.uint64).reshape(len(recs), nw)
    counts = np.array([r[1] for r in recs], dtype=np.uint32)
    order = rng.permutation(len(recs))
    if len(recs):
        dk = torch.from_numpy(np.ascontiguousarray(keys[order]).view(np.int64)).cuda()
        dc = torch.from_numpy(np.ascontiguousarray(counts[order]).view(np.int32)).cuda()
    else:  # no record: the arrays are not read, but a set with counts needs a counts pointer
        dk, dc = torch.zeros(nw, dtype=torch.int64).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    s = ctx.kmerset_from_device(dk, len(recs), k, d_counts=dc, flags=B.CANONICAL)
    assert len(s) == len(recs)
    if len(recs):
        got_k, got_c = s.export(with_counts=True)
        assert got_k.tobytes() == keys.tobytes() and got_c.astype(np.uint32).tobytes() == counts.tobytes()
    return s, (keys, counts)


@pytest.mark.parametrize("k", [31, 32, 33, 63, 64, 65, 96, 97, 127])
def test_join_of_crafted_samples(ctx, torch_device, tmp_path, k):
    rng = np.random.default_rng(k)
    for union in (128, 129):
        for ci, cs in ((3, 255), (1, 1000), (2, 65535)):
            samples = _join_samples(k, union, ci, cs, seed=0)
            sets, exported = zip(*[_device_set(ctx, k, s, rng) for s in samples])
            assert len(sets[2]) == 0 and max(exported[3][1]) < ci
            d = tmp_path / ("u%d_cs%d" % (union, cs))
            d.mkdir()
            _, rk, rr = check_profile_join(ctx, d, k, sets, exported, 1, min_mult=MIN_MULT, ci=ci, cs=cs)
            table = dict(zip(rk, rr))
            # everything a sample holds at ci or above survives its filter: the union is whole before the keep rule
            _, rk0, _ = check_profile_join(ctx, d, k, sets, exported, 0, min_mult=0, ci=ci, cs=cs)
            assert len(rk0) == union == len({km for s in samples for km, c in s.items() if c >= ci})
            # one sample present: total == MIN_MULT goes, MIN_MULT + 1 stays; the values are saturated at cs
            lone = {min(c, cs): R.encode(km) for km, c in samples[0].items()
                    if km not in samples[1] and c >= ci}
            assert MIN_MULT + 1 in lone and table[lone[MIN_MULT + 1]] == [MIN_MULT + 1, 0, 0, 0]
            if ci <= MIN_MULT:
                assert MIN_MULT in lone and lone[MIN_MULT] not in table
            assert cs in lone and table[lone[cs]] == [cs & 0xFFFF, 0, 0, 0]
            if ci == 1:  # two samples present with a total of 2
                ones = [R.encode(km) for km, c in samples[0].items() if c == 1 and samples[1].get(km) == 1]
                assert ones and all(table[key] == [1, 1, 0, 0] for key in ones)
            # the keep rule at min_mult = cs - 1 and cs, two samples required, and all N of them (one is empty)
            check_profile_join(ctx, d, k, sets, exported, 1, min_mult=cs - 1, ci=ci, cs=cs)
            _, rkc, _ = check_profile_join(ctx, d, k, sets, exported, 1, min_mult=cs, ci=ci, cs=cs)
            assert rkc and all(sum(1 for v in table[key] if v) > 1 for key in rkc)
            _, rk2, _ = check_profile_join(ctx, d, k, sets, exported, 2, min_mult=MIN_MULT, ci=ci, cs=cs)
            assert 0 < len(rk2) < len(rk)
            _, rk4, _ = check_profile_join(ctx, d, k, sets, exported, N_JOIN, min_mult=MIN_MULT, ci=ci, cs=cs)
            assert rk4 == []
            d2 = d / "two"
            d2.mkdir()
            _, rkn, rrn = check_profile_join(ctx, d2, k, sets[:2], exported[:2], 2, min_mult=MIN_MULT, ci=ci, cs=cs)
            assert rkn == rk2 and all(all(row) for row in rrn)  # min_samples = N with every sample holding k-mers
            # the families that differ in their last base (k > 32: in their last word) only stay apart
            fam = rk0
            heads = [key[:-1] if len(key) > 1 else key[0] & ((1 << (2 * k - 2)) - 1) for key in fam]
            assert len(heads) - len(set(heads)) >= 2
