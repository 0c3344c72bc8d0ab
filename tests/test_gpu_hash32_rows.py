"""GPU: stage A's narrow dedup kernel (k_bucket_hash32, msd_narrow_a.h) row by row.

In slot mode the kernel walks a bucket of n <= 8192 records in four rows of 2048 (a lane holds records
4 * (r * 512 + tid) .. + 3 of row r, loaded as one uint4): a row past n is skipped, a row below n runs without
per-record predicates, the last one tests its records; the lanes whose first slot held another key walk on in a loop of
their own, which is also where a bucket is given up.  What can go wrong sits at the row edges, in the last group of
four and in that loop, so the cases are chosen by the FILLS of their buckets.

Sweep: CANONICAL | UNSORTED at k = 17, 19, 21 over 150 bp reads of a 200 kb genome, every case in a fresh process with
poisoned device memory (BBK_POOL_POISON: the tail of a slot past n holds 0xCD bytes), compared as a sorted set with the
canonical set of the oracle's result.  Every run restates nw_mix, nw_bin1 and the level-2 bin in numpy and computes the
fill of every bucket from the oracle's multiplicities (the both-strand count of a canonical k-mer is the number of its
instances in the reads); the plan is checked by its bucket count against the BBK_VERBOSE line.  Uniform reads between
3 000 and 60 000 give buckets of 290 .. 5 734 records (a segment above 0.70 * 8192 records is split), on either side of
2048 and 4096 and with every n mod 4 -- but never a fill below 4 or at 6144.  Two cases add those: 25 reads (3 300
instances over 1024 buckets: hundreds of buckets of one to three records), and 60 000 reads plus 2 700 copies of the
first one, whose ~130 k-mers lift their buckets from ~3 800 to ~6 500 records (some beyond the slot: those buckets take
the overflow path).

Payload: the extension index at k = 21 drives OP = 3 (mask bytes OR-ed per key) through the same front half.
Forced give-up: BBK_HASH_MAX_PROBES=2 ends the walk of a record at its third slot; the buckets that hold such a record
are given up and reprocessed, the others finish -- the result must still be the oracle's.
"""
import functools
import os
import re
import subprocess
import sys

import pytest

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("BBK_DISABLE_MSD")), reason="tests of the MSD path's modes")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENOME = 200000
SWEEP = [(3000, 0), (16000, 0), (30000, 0), (44000, 0), (60000, 0)]  # (reads, copies of the first read added)
EDGES = [(25, 0), (60000, 2700)]
KS = (17, 19, 21)

SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import spades_for_blackbird_amd as B
from oracle import oracle as O
from tests.helpers import synth_reads

M32 = np.uint64(0xFFFFFFFF)

def nw_mix(lo):
    t = (lo * np.uint64(0x9E3779B1)) & M32
    t ^= t >> np.uint64(15)
    t = (t * np.uint64(0x85EBCA6B)) & M32
    t ^= t >> np.uint64(13)
    return t

def msb_first(x, k):  # base 0 most significant: numeric order = base-lexicographic order
    r = np.zeros_like(x)
    for i in range(k):
        r = (r << np.uint64(2)) | ((x >> np.uint64(2 * i)) & np.uint64(3))
    return r

def is_canonical(x, k):  # the reverse complement of x is the complement of x read backwards
    m = msb_first(x, k)
    return m <= msb_first(m ^ np.uint64((1 << (2 * k)) - 1), k)

def bucket_fills(keys, counts, k):
    # msd_narrow_a.h: segment = nw_bin1(hi, mix(lo)), level-2 bin = ((mix & 0x3FFFFF) * nb) >> 22; msd.hip
    # level2_layout: nb = ceil(segment fill / (0.70 * 8192)) bins per segment
    hb = 2 * k - 32
    lo, hi = keys & M32, keys >> np.uint64(32)
    t = nw_mix(lo)
    seg = ((t >> np.uint64(22)) ^ (hi << np.uint64(10 - hb))).astype(np.int64)
    h1 = np.bincount(seg, weights=counts, minlength=1024)
    nb = np.minimum(1024, np.maximum(1, np.ceil(h1 / (0.70 * 8192)))).astype(np.uint64)
    first = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    b = (((t & np.uint64(0x3FFFFF)) * nb[seg]) >> np.uint64(22)).astype(np.int64)
    return np.bincount(first[seg] + b, weights=counts, minlength=int(first[-1])).astype(np.int64)

ctx = B.Context(0)
n, dup = %(n)d, %(dup)d
reads = synth_reads(n, read_len=150, genome_len=%(g)d, sub_rate=0.01, seed=5)
reads += [reads[0]] * dup
whole = ctx.reads_from_ascii(reads)
for k in %(ks)r:
    sys.stderr.write("CASE %%d\n" %% k)
    sys.stderr.flush()
    if %(ext)d:
        ox = O.ExtIndex(reads, k, 1)
        order = np.lexsort([ox.kmers[:, j] for j in range(ox.kmers.shape[1] - 1, -1, -1)])
        x = ctx.extindex(whole, k)
        xk, xm = x.export()
        assert np.array_equal(xk, ox.kmers[order]) and np.array_equal(xm, ox.masks[order]), ("extension index", k)
        continue
    both, cnt = O.kmercount(reads, k, 16, 2, with_counts=True)
    keep = is_canonical(both[:, 0], k)
    exp = np.sort(both[keep, 0])
    assert 2 * len(exp) == len(both), k
    u = ctx.count(whole, k, B.CANONICAL | B.UNSORTED)
    got, _ = u.export_by_owner(1)
    assert np.array_equal(np.sort(got[:, 0]), exp), (n, k, len(got), len(exp))
    u.free()
    f = bucket_fills(both[keep, 0], cnt[keep].astype(np.float64), k)
    print("FILLS", k, len(f), *sorted(set(int(v) for v in f[f > 0])))
print("HASH32-OK")
"""


@functools.lru_cache(maxsize=None)
def _run(n, dup, ks=KS, ext=False, max_probes=None):
    """one fresh process: ({k: verbose lines of that call}, {k: (buckets of the restated plan, its distinct non-zero
    fills)})"""
    env = dict(os.environ, BBK_VERBOSE="1", BBK_POOL_POISON="1", BBK_SLOTS_MIN="0")
    env.pop("BBK_HASH_MAX_PROBES", None)
    if max_probes is not None:
        env["BBK_HASH_MAX_PROBES"] = str(max_probes)
    script = SCRIPT % {"root": ROOT, "g": GENOME, "n": n, "dup": dup, "ks": tuple(ks), "ext": int(ext)}
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "HASH32-OK" in r.stdout
    lines, cur = {}, None
    for l in r.stderr.splitlines():
        m = re.match(r"CASE (\d+)$", l)
        if m:
            cur = int(m.group(1))
            lines[cur] = []
        elif cur is not None and "[bbk]" in l:
            lines[cur].append(l)
    fills = {}
    for l in r.stdout.splitlines():
        if l.startswith("FILLS"):
            v = [int(x) for x in l.split()[1:]]
            fills[v[0]] = (v[1], v[2:])
    return lines, fills


def _slots_line(lines):
    """(buckets, spilled records, overflowing buckets) of the narrow slot pass"""
    for l in lines:
        m = re.search(r"msd slots \(narrow records\) N=\d+ nb1=1024 seg_cap=\d+ buckets=(\d+) spill=(\d+) over_seg=\d+ over_bkt=(\d+)", l)
        if m:
            return int(m.group(1)), int(m.group(2)), int(m.group(3))
    return None


@pytest.mark.parametrize("n,dup", SWEEP + EDGES)
def test_rows_equal_the_oracle(n, dup):
    """one size: the canonical set equals the oracle's at k = 17, 19, 21 (asserted inside the run) on the narrow slot
    route, and the restated plan has exactly the buckets the call reports -- so its fills are the fills the kernel saw;
    without added copies nothing spills, no bucket overflows its slot or is given up"""
    lines, fills = _run(n, dup)
    for k in KS:
        s = _slots_line(lines[k])
        assert s is not None, (n, k, lines[k])
        assert fills[k][0] == s[0], (n, k, fills[k][0], lines[k])
        if not dup:
            assert s[1] == 0 and s[2] == 0, (n, k, lines[k])
            assert max(fills[k][1]) <= 5735, (n, k, max(fills[k][1]))  # a fuller segment is split


def test_sweep_reaches_the_row_edges():
    """the fills of the sweep as a whole: every n mod 4, a fill below 4, and fills within a quarter row on either side
    of 2048, 4096 and 6144"""
    seen = set()
    for n, dup in SWEEP + EDGES:
        _, fills = _run(n, dup)
        for k in KS:
            seen.update(fills[k][1])
    assert {f % 4 for f in seen} == {0, 1, 2, 3}
    assert any(f < 4 for f in seen)
    for edge in (2048, 4096, 6144):
        assert any(edge - 512 <= f < edge for f in seen) and any(edge <= f < edge + 512 for f in seen), edge


def test_payload_through_the_shared_front_half():
    """the extension index at k = 21 (OP = 3: one mask byte per record, OR-ed per key) against the oracle's"""
    lines, _ = _run(16000, 0, ks=(21,), ext=True)
    assert any("msd slots (narrow records)" in l for l in lines[21]), lines[21]


def test_forced_give_up_in_the_walk():
    """BBK_HASH_MAX_PROBES=2: a record that needs a third slot gives its bucket up; such buckets are reprocessed,
    the result equals the oracle's (asserted inside the run)"""
    lines, _ = _run(16000, 0, ks=(21,), max_probes=2)
    s = _slots_line(lines[21])
    assert s is not None and s[2] > 0, lines[21]
