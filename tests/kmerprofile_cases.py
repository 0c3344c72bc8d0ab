"""Crafted inputs for the tests of the k-mer profile engine (tests/test_kmerprofile_cases.py on the CPU,
tests/test_gpu_kmerprofile_edges.py on the GPU): contigs and a profile table (canonical k-mer string -> row of u16
values) built so that every contig finds an exact number n of its k-mers and every column of its rows belongs to one
class of values.  A case is a dict:

    k, N, contigs [(name, sequence)], table {canonical k-mer: row}, n {name: k-mers found}, hits {name: the found
    canonical k-mers in contig order}

Nothing here depends on the engine; every expectation comes from tests/kmerprofile_restated.py.
"""
import functools

import numpy as np

from tests import kmerprofile_restated as R

CLASSES = ("equal", "low", "straddle", "ties", "extremes", "bytes", "zero")
N_SAMPLES = len(CLASSES)
# the number of found k-mers of the plain contigs: the steps of the winsor offset (20/21, 40/41), the 64-lane rounds
PLAIN_N = (2, 3, 19, 20, 21, 63, 65, 128, 1000)


def _genome(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def column(cls, n, rng, eight=False):
    """n values of one class, in the order the contig finds them.  eight: the same classes inside one byte"""
    top, half, t = (255, 128, 70) if eight else (65535, 256, 700)
    if n == 0:
        return []
    o = R.winsor_offset(n)

    def shuffled(v):
        v = [int(x) for x in v]
        return [v[i] for i in rng.permutation(len(v))]
    if cls == "equal":
        return [30 if eight else 300] * n
    if cls == "zero":
        return [0] * n
    if cls == "low":
        return [int(x) for x in rng.integers(0, 16 if eight else 256, n)]
    if cls == "bytes":
        pool = (15, 16, 31, 32, 47, 48) if eight else (255, 256, 511, 512, 767, 768)
        return [int(pool[i]) for i in rng.integers(0, len(pool), n)]
    if cls == "straddle":  # sorted[o] < half <= sorted[n - o - 1] from n = 4 on
        lo_n = (n + 1) // 2
        return shuffled(list(rng.integers(0, half, lo_n)) + list(rng.integers(half, min(8 * half, top + 1), n - lo_n)))
    if cls == "extremes":  # the o smallest are 0, the o largest are the top value
        if n < 3:
            return [top] if n == 1 else [0, top]
        return shuffled([0] * o + [top] * o + list(rng.integers(1, top, n - 2 * o)))
    if cls == "ties":  # exactly o values below a run of t, exactly o values above a run of t + 1
        if n < 4:
            return [[t], [t + 1, t], [top, t, 0]][n - 1]
        a = (n - 2 * o + 1) // 2
        b = n - 2 * o - a
        rest = list(rng.integers(0, t, o)) + list(rng.integers(t + 2, top + 1, o))
        head, mid = [], []
        if a > 64:  # one 64-lane round of equal values in front, another at 128..191: uniform and mixed rounds in one column
            head, a = [t] * 64, a - 64
        if b > 64 and n >= 256:
            mid, b = [t + 1] * 64, b - 64
        rest = shuffled(rest + [t] * a + [t + 1] * b)
        if mid:
            rest = rest[:128 - len(head)] + mid + rest[128 - len(head):]
        return head + rest
    raise ValueError(cls)


def _piece(rng, k, hits):
    """(sequence, hit flags): a random stretch with one k-mer position per flag"""
    return _genome(rng, len(hits) + k - 1), list(hits)


def _contig_specs(k, rng):
    """[(name, [pieces])]: piece = (sequence, hit flag per position); a piece shorter than k has no flags"""
    T, F = [True], [False]
    specs = [("n%d" % n, [_piece(rng, k, T * n)]) for n in PLAIN_N]
    specs += [
        ("lane63", [_piece(rng, k, F * 63 + T + F * 6)]),  # n = 1: the single hit of a round sits in its last lane
        ("alt40", [_piece(rng, k, (T + F) * 40)]),
        ("alt64", [_piece(rng, k, (F + T) * 64)]),
        ("late41", [_piece(rng, k, F * 64 + T * 41)]),  # the first round finds nothing
        ("n127", [_piece(rng, k, T * 127)]),
        ("short129", [_piece(rng, k, T * 64), (_genome(rng, min(k - 1, 5)), []), _piece(rng, k, T * 65)]),
        # the running count crosses the 64-entry rounds at offsets 1, 64, 128, 193
        ("cut257", [_piece(rng, k, T * p) for p in (1, 63, 64, 65, 64)]),
        ("share70", [_piece(rng, k, T * 35 + F * 30 + T * 35)]),  # 70 of 100 positions: gets a line
        ("share69", [_piece(rng, k, T * 35 + F * 31 + T * 34)]),  # 69 of 100: gets none
        ("mixed", [_piece(rng, k, [bool(x) for x in rng.integers(0, 2, 300)])]),
        ("none", [_piece(rng, k, F * 100)]),
        ("nopiece", []),
    ]
    return specs


def _finish(k, contigs, hits, rng, eight, extra_keys=()):
    table = {}
    for name, _ in contigs:
        found = hits[name]
        new = [km for km in dict.fromkeys(found) if km not in table]  # a contig given twice (its reverse complement)
        cols = [column(cls, len(new), rng, eight) for cls in CLASSES]
        for i, km in enumerate(new):
            table[km] = [c[i] for c in cols]
    for km in extra_keys:  # keys no contig holds
        assert km not in table
        table[km] = [int(x) for x in rng.integers(1, 256 if eight else 65536, N_SAMPLES)]
    return dict(k=k, N=N_SAMPLES, contigs=contigs, table=table, hits=hits, n={c: len(h) for c, h in hits.items()})


@functools.lru_cache(maxsize=None)
def crafted(k, seed=0, eight=False):
    """the crafted profile of one k >= 15: 22 contigs (154 columns: the last block of the reduction holds idle waves)"""
    assert k >= 15
    rng = np.random.default_rng([k, seed])
    contigs, hits, misses = [], {}, []
    for ci, (name, pieces) in enumerate(_contig_specs(k, rng)):
        seq, found = "", []
        for pi, (s, flags) in enumerate(pieces):
            seq += ("" if pi == 0 else "N" * (1 + (pi + ci) % 2)) + s
            for j, hit in enumerate(flags):
                (found if hit else misses).append(R.canonical(s[j:j + k]))
        if name == "nopiece":
            seq = "NNNN"
        contigs.append((name, seq))
        hits[name] = found
    allk = [km for h in hits.values() for km in h] + misses
    assert len(set(allk)) == len(allk), "the contigs' k-mers must be distinct"
    rc_of = dict(contigs)["n127"]
    contigs.append(("rc127", R.rc(rc_of)))
    hits["rc127"] = hits["n127"][::-1]
    # keys no contig holds that equal a missed k-mer in every word but the last: its last base changed
    known, near = set(allk), []
    for km in misses:
        for b in "ACG":
            cand = km[:-1] + b
            if b != km[-1] and R.canonical(cand) == cand and cand not in known and R.rc(cand) not in known:
                near.append(cand)
                known.add(cand)
                break
        if len(near) == 24:
            break
    assert len(contigs) == 22 and (len(contigs) * N_SAMPLES) % 4 != 0
    case = _finish(k, contigs, hits, rng, eight, near)
    case["near"] = near
    return case


def restricted(case, n_keys):
    """the same contigs over n_keys keys from the middle of the table: most queries fall below the first key, above the
    last key or into empty bins of the prefix table"""
    keys = sorted(case["table"], key=R.encode)
    first = (len(keys) - n_keys) // 2
    keep = set(keys[first:first + n_keys])
    hits = {c: [km for km in h if km in keep] for c, h in case["hits"].items()}
    return dict(case, table={km: case["table"][km] for km in keep}, hits=hits, n={c: len(h) for c, h in hits.items()})


def shared_bases(k):
    """[first, last): the 12 bases under the top 24 populated bits of word 0"""
    hi = min(k, 32)
    return hi - 12, hi


@functools.lru_cache(maxsize=None)
def clustered(k, seed=0, eight=False):
    """every key (and every query) shares the bases under the top bits of word 0: one bin of the prefix table holds the
    whole table.  The k-mers begin with A and end in A, C or G, which makes them canonical; every piece of the two
    contigs is one k-mer, the second contig gives every other one as its reverse complement."""
    rng = np.random.default_rng([k, seed, 1])
    lo, hi = shared_bases(k)
    fixed = "GATTACAGTCAC"

    def kmer():
        s = "A" + _genome(rng, k - 2) + "ACG"[int(rng.integers(0, 3))]
        return s[:lo] + fixed + s[hi:]
    kms = list(dict.fromkeys(kmer() for _ in range(170)))
    assert all(R.canonical(km) == km for km in kms)
    one, two, miss = kms[:100], kms[100:140], kms[140:]
    near = []
    if R.words(k) > 1:  # misses that equal a key in every word but the last
        near = [km[:-1] + "ACG"[("ACG".index(km[-1]) + 1) % 3] for km in one[:10]]
        near = [km for km in near if km not in kms]
    pieces1, pieces2 = [], []
    for i, km in enumerate(one):
        pieces1.append(km)
        if i % 3 == 2:
            pieces1.append((miss + near)[(i // 3) % len(miss + near)])
    for i, km in enumerate(two):
        pieces2.append(R.rc(km) if i % 2 else km)
    for i, km in enumerate(near):
        pieces2.append(R.rc(km) if i % 2 else km)
    contigs = [("cluster100", "N".join(pieces1)), ("cluster40", "NN".join(pieces2))]
    case = _finish(k, contigs, {"cluster100": one, "cluster40": two}, rng, eight)
    case["miss"] = miss + near
    return case


@functools.lru_cache(maxsize=None)
def small_k(k, seed=0):
    """k = 1 .. 4: a table over all (odd k) or every other (even k) canonical k-mer, rows drawn from the classes' values;
    k-mers repeat along the contigs, n is simply the number of positions that find a row"""
    assert 1 <= k <= 4
    rng = np.random.default_rng([k, seed, 2])
    canon = sorted({R.canonical("".join("ACGT"[(i >> (2 * j)) & 3] for j in range(k))) for i in range(4 ** k)})
    keys = canon if k % 2 else canon[::2]
    pool = (0, 1, 255, 256, 300, 511, 512, 700, 701, 65535)
    table = {km: [int(pool[i]) for i in rng.integers(0, len(pool), N_SAMPLES)] for km in keys}
    contigs = [("one", _genome(rng, k)), ("five", _genome(rng, 5 + k - 1)), ("r64", _genome(rng, 64 + k - 1)),
               ("r65", _genome(rng, 65 + k - 1)), ("long", _genome(rng, 300)),
               ("cut", _genome(rng, 70) + "N" + _genome(rng, max(k - 1, 1)) + "NN" + _genome(rng, 63 + k - 1)),
               ("poly", "A" * 130), ("empty", "N")]
    hits = {}
    for name, seq in contigs:
        hits[name] = [c for p in R.split_on_ns(seq) for c in (R.canonical(p[j:j + k]) for j in range(len(p) - k + 1))
                      if c in table]
    return dict(k=k, N=N_SAMPLES, contigs=contigs, table=table, hits=hits, n={c: len(h) for c, h in hits.items()})


def table_files(case):
    """(keys sorted as word tuples, rows, bytes of <prefix>.kmers, bytes of <prefix>.bpr)"""
    keys = sorted(R.encode(km) for km in case["table"])
    rows = [case["table"][R.decode(key, case["k"])] for key in keys]
    return keys, rows, R.kmers_bytes(keys), R.bpr_bytes(rows)


def pieces_of(contigs):
    """(pieces, first_piece): what Context.reads_from_ascii and KmerProfile.abundance take"""
    pieces, first = [], [0]
    for _, seq in contigs:
        pieces += R.split_on_ns(seq)
        first.append(len(pieces))
    return pieces, first


def expected(case):
    """[(n, positions, sums, sums of squares)] per contig, from the restatement"""
    return [R.abundance_ints(seq, case["k"], case["table"], case["N"]) for _, seq in case["contigs"]]
