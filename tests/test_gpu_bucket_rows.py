"""GPU: the sort kernel of narrow stage B pays for the rows a bucket holds (k_bucket_dist_nb); stage A's narrow dedup
(k_bucket_hash32) over buckets from nearly empty to nearly full.

k_bucket_dist_nb walks a bucket in rows of 512 records (record p = row * 512 + lane) and runs every per-row phase for
rows < ceil(n / 512) only (a ranking round of two rows as a whole); it stores its sorted bucket position by position and
only reports whether two neighbours were equal.  k_bucket_hash32 is as it was (a row bound and a compact copy-out were
measured and not kept, DESIGN 4.4 "Bucket kernels (round 9)"); its sweep stays as a check of that kernel at uneven fills.

Stage B: BOTH_STRANDS and BOTH_STRANDS | REFERENCE_ORDER at k = 15 and 17 (the sizes at which
tests/test_gpu_stage_b_narrow.py shows the 4-byte key-slot route running) over six read counts, every case equal to the
oracle and byte-equal to the BBK_NO_NARROW_B=1 run (8-byte records, k_bucket_dist), in fresh processes with poisoned
device memory.  The route is asserted from the BBK_VERBOSE lines.  What the read count can do to the mean fill
(N / buckets of the "ordered without histograms" line) is limited by the planner, which this file leaves alone: it aims
every bucket at 0.70 * 5632 = 3942 records whatever N is, so the means of the sweep stay a little below that (seven or
eight rows; single buckets reach nine) -- except the tagged order at k = 17, which takes 16 384 buckets of a few dozen records (one partial row).
A mean above 4096 cannot be planned.  The fills of the single buckets are therefore computed: for the ascending order
the run repeats the key-slot plan on the oracle's keys (plan_fills: level-1 segments by the top bits of the key, bins
per segment from the segment's fill, bin = floor(q * nb / P)), the bucket count of that plan must equal the one the
verbose line reports, and the rows of every bucket, ceil(fill / 512), are what the tests assert on.  All eleven rows,
and with them the last ranking round (the one whose second slot lies past ITEMS), are reached by one bucket of its own
case: 1900 reads of 17 bases that share their last five put 1900 distinct keys into a range a quarter of a bucket wide
(the last bases are a key's top bits), and the plan shows a bucket of more than 5120 and at most 5632 records.

Stage A: CANONICAL | UNSORTED at k = 17, 19, 21 over the same read counts and one more, compared as a sorted set with
the canonical set of the oracle's result.  Its 1024 (later 2048) buckets hold 380 to 4900 records on average, on
either side of 512, 1024 and 2048 in consecutive cases, and far from evenly (the ~15 copies of a k-mer share a bucket).
One input adds reads that begin with T x 16.  A canonical k-mer of k < 32 cannot begin with sixteen T (its reverse
complement, which ends in A x 16, is the smaller of the two), so the all-ones record -- the table's empty marker --
cannot arise from reads at these k; the reads are there so that this stays pinned, and their reverse complements
pass through the kernel like any record.

No public entry point reaches k_bucket_dist_nb with a real duplicate: the kernel runs only on the expansion of a set the
dedup of stage A made distinct, at odd k, where a k-mer never equals its reverse complement.  Its duplicate verdict is
checked on the host (tests/bucket_tail_check.cpp); here every case asserts that no duplicate was reported.
"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("BBK_DISABLE_MSD")), reason="tests of the MSD path's modes")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GENOME = 200000
# reads of 150 bp over a 200 kb genome, 1 % substitutions
SWEEP = [3000, 4000, 8000, 16000, 30000, 60000]
FULL = (16000, 1900)  # reads, and reads of 17 bases sharing their last five: one bucket of eleven rows at k = 17
STAGE_A = [3000, 4000, 8000, 16000, 38000, 60000]

SCRIPT_B = r"""
import hashlib, math, sys
import numpy as np
sys.path.insert(0, %(root)r)
import spades_for_blackbird_amd as B
from oracle import oracle as O
from tests.helpers import synth_reads

def plan_fills(keys, k):
    # bucket fills of the key-slot plan (msd.hip: plan, level2_layout; msd_part.h: prefix_of, bin_of) for the
    # ascending order of `keys`
    target = 0.70 * 5632
    want = max(1.0, math.ceil(len(keys) / target))
    nb1, b1 = 1, 0
    while nb1 < 512 and nb1 * nb1 < want:
        nb1, b1 = nb1 << 1, b1 + 1
    p = (keys << np.uint64(64 - 2 * k)) >> np.uint64(32)
    seg = (p >> np.uint64(32 - b1)).astype(np.int64)
    h1 = np.bincount(seg, minlength=nb1)
    nb2 = np.minimum(1024, np.maximum(1, np.ceil(h1 / target))).astype(np.uint64)
    sbin = np.concatenate([[0], np.cumsum(nb2)]).astype(np.int64)
    rest = (p << np.uint64(b1)) & np.uint64(0xFFFFFFFF)
    b = ((rest * nb2[seg]) >> np.uint64(32)).astype(np.int64)
    return np.bincount(sbin[seg] + b, minlength=int(sbin[-1]))

ctx = B.Context(0)
check = %(check)r
for n in %(ns)r:
    reads = synth_reads(n, read_len=150, genome_len=%(g)d, sub_rate=0.01, seed=5)
    if %(hot)d:
        rng = np.random.default_rng(21)
        reads += ["".join("ACGT"[x] for x in t) + "ACGTT" for t in rng.integers(0, 4, size=(%(hot)d, 12))]
    if %(skew)r:
        # reads of exactly k bases sharing their first eleven: they crowd one distribution bin of their buckets
        rng = np.random.default_rng(9)
        tails = rng.integers(0, 4, size=(6000, 17 - 11))
        reads += ["ACGTTGCAAGT" + "".join("ACGT"[x] for x in t) for t in tails]
    whole = ctx.reads_from_ascii(reads)
    for k in %(ks)r:
        exp = O.kmercount(reads, k, 16, 2) if check else None
        for flags, name in ((B.BOTH_STRANDS | B.REFERENCE_ORDER, "ref"), (B.BOTH_STRANDS, "plain")):
            sys.stderr.write("CASE %%d %%d %%s\n" %% (n, k, name))
            sys.stderr.flush()
            s = ctx.count(whole, k, flags)
            got = s.export(B.ORDER_REFERENCE_BUCKETS16 if name == "ref" else B.ORDER_SORTED)
            if check:
                e = exp if name == "ref" else np.sort(exp[:, 0]).reshape(-1, 1)
                assert np.array_equal(got, e), (n, k, name, len(got), len(e))
                if name == "plain":
                    f = plan_fills(e[:, 0], k)
                    print("FILLS", n, k, len(f), int(f.max()), *sorted(set(int(x) for x in -(-f // 512))))
            print("HASH", n, k, name, len(got), hashlib.sha256(got.tobytes()).hexdigest())
            s.free()
print("ROWS-B-OK")
"""

SCRIPT_A = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import spades_for_blackbird_amd as B
from oracle import oracle as O
from tests.helpers import synth_reads

def msb_first(x, k):  # base 0 most significant: numeric order = base-lexicographic order
    r = np.zeros_like(x)
    for i in range(k):
        r = (r << np.uint64(2)) | ((x >> np.uint64(2 * i)) & np.uint64(3))
    return r

def canonical(x, k):  # the reverse complement of x is the complement of x read backwards
    m = msb_first(x, k)
    rc = m ^ np.uint64((1 << (2 * k)) - 1)
    return np.where(m <= msb_first(rc, k), x, rc)

ctx = B.Context(0)
rng = np.random.default_rng(3)
for n in %(ns)r:
    reads = synth_reads(n, read_len=150, genome_len=%(g)d, sub_rate=0.01, seed=5)
    if n == %(ns)r[1]:
        reads += ["T" * 16 + "".join("ACGT"[x] for x in rng.integers(0, 4, size=40)) for _ in range(50)]
        reads += ["T" * 40]
    whole = ctx.reads_from_ascii(reads)
    for k in (17, 19, 21):
        both = O.kmercount(reads, k, 16, 2)[:, 0]
        exp = np.unique(canonical(both, k))
        assert 2 * len(exp) == len(both), (n, k)
        for x in exp[:: max(1, len(exp) // 40)]:  # the rule above against the oracle's own test of a k-mer
            assert O.kmer_is_minimal("".join("ACGT"[(int(x) >> (2 * i)) & 3] for i in range(k))), (n, k, hex(int(x)))
        sys.stderr.write("CASE %%d %%d canon\n" %% (n, k))
        sys.stderr.flush()
        u = ctx.count(whole, k, B.CANONICAL | B.UNSORTED)
        got, _ = u.export_by_owner(1)
        assert np.array_equal(np.sort(got[:, 0]), exp), (n, k, len(got), len(exp))
        u.free()
print("ROWS-A-OK")
"""


def _cases(err):
    """{(reads, k, name): [verbose lines of that call]}"""
    out, cur = {}, None
    for line in err.splitlines():
        m = re.match(r"CASE (\d+) (\d+) (\w+)$", line)
        if m:
            cur = (int(m.group(1)), int(m.group(2)), m.group(3))
            out[cur] = []
        elif cur is not None and "[bbk]" in line:
            out[cur].append(line)
    return out


def _run(script, args, marker, narrow=True):
    env = dict(os.environ, BBK_VERBOSE="1", BBK_POOL_POISON="1", BBK_SLOTS_MIN="0")
    env.pop("BBK_NO_NARROW_B", None)
    if not narrow:
        env["BBK_NO_NARROW_B"] = "1"
    r = subprocess.run([sys.executable, "-c", script % dict({"hot": 0}, **args, root=ROOT, g=GENOME)], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert marker in r.stdout
    fills = {}  # (reads, k) -> (buckets of the plan, largest bucket, set of rows its buckets take)
    for l in r.stdout.splitlines():
        if l.startswith("FILLS"):
            v = [int(x) for x in l.split()[1:]]
            fills[(v[0], v[1])] = (v[2], v[3], set(v[4:]))
    return [l for l in r.stdout.splitlines() if l.startswith("HASH")], _cases(r.stderr), fills


def _width(lines):
    for l in lines:
        m = re.search(r"msd key slots: (\d)-byte records", l)
        if m:
            return m.group(1) + "-byte"
    return None


def _ordered(lines):
    """(N, buckets) of the line that says the key slots held"""
    for l in lines:
        m = re.search(r"msd key slots N=(\d+) buckets=(\d+): ordered without histograms", l)
        if m:
            return int(m.group(1)), int(m.group(2))
    return None


@pytest.fixture(scope="module")
def stage_b():
    """the whole sweep once on each route: (hashes, verbose lines, plan fills) of the 4-byte run (checked against the
    oracle) and of the 8-byte run"""
    args = {"ns": SWEEP, "ks": (15, 17), "skew": False}
    return _run(SCRIPT_B, dict(args, check=True), "ROWS-B-OK"), _run(SCRIPT_B, dict(args, check=False), "ROWS-B-OK", False)


@pytest.mark.parametrize("n", SWEEP)
def test_sort_kernel_rows(stage_b, n):
    """one size of the sweep: oracle-equal (asserted inside the run), byte-equal to the 8-byte route, on the 4-byte
    route, no bucket turned down and no duplicate reported; the plan repeated on the oracle's keys has the buckets the
    call reports"""
    (h4, c4, fills), (h8, c8, _) = stage_b
    mine = [l for l in h4 if l.split()[1] == str(n)]
    assert len(mine) == 4 and mine == [l for l in h8 if l.split()[1] == str(n)]
    for k in (15, 17):
        for name in ("ref", "plain"):
            lines = c4[(n, k, name)]
            assert _width(lines) == "4-byte", (n, k, name, lines)
            assert not any("given up" in l for l in lines), lines
            assert _ordered(lines) is not None, lines
            assert _width(c8[(n, k, name)]) in ("8-byte", None), c8[(n, k, name)]
        assert fills[(n, k)][0] == _ordered(c4[(n, k, "plain")])[1], (n, k, fills[(n, k)], c4[(n, k, "plain")])


def test_sort_kernel_sweep_reaches_small_and_middle_rows(stage_b):
    """the sweep as a whole: buckets of one partial row (the tagged order at k = 17, by its mean), buckets of seven,
    eight and nine rows (ascending order, per bucket, from the plan), and means on either side of 7 * 512"""
    (_, c4, fills), _ = stage_b
    means = [N / nb for N, nb in (_ordered(lines) for lines in c4.values())]
    assert min(means) < 512
    assert any(3072 < m <= 3584 for m in means) and any(3584 < m <= 4096 for m in means), sorted(means)
    rows = set().union(*(r for _, _, r in fills.values()))
    assert {7, 8, 9} <= rows, rows


def test_sort_kernel_all_eleven_rows():
    """one bucket past 5120 records, inside its slot of 5632: all eleven rows and every ranking round run, the bucket
    is not turned down, and the result is the oracle's and the 8-byte route's"""
    n, hot = FULL
    args = {"ns": [n], "ks": (17,), "skew": False, "hot": hot}
    h4, c4, fills = _run(SCRIPT_B, dict(args, check=True), "ROWS-B-OK")
    h8, _, _ = _run(SCRIPT_B, dict(args, check=False), "ROWS-B-OK", False)
    assert h4 == h8
    lines = c4[(n, 17, "plain")]
    assert _width(lines) == "4-byte" and not any("given up" in l for l in lines), lines
    nb, largest, rows = fills[(n, 17)]
    assert nb == _ordered(lines)[1], (nb, lines)
    assert 5120 < largest <= 5632 and 11 in rows, (largest, rows)


def test_dedup_kernel_over_uneven_fills():
    """stage A's narrow dedup over the sweep's read counts (the asserts are inside the run), on the 4-byte route"""
    _, cases, _ = _run(SCRIPT_A, {"ns": STAGE_A}, "ROWS-A-OK")
    assert len(cases) == 3 * len(STAGE_A)
    for case, lines in cases.items():
        assert any("msd slots (narrow records)" in l for l in lines), (case, lines)


def test_turned_down_bucket_at_a_partial_row_size():
    """the crowded bin of test_narrow_stage_b_give_up_to_exact_mode at another size of the sweep: the sort kernel turns
    those buckets down, the call goes to the exact mode, the result equals the oracle and the 8-byte route's"""
    n = SWEEP[2]
    args = {"ns": [n], "ks": (17,), "skew": True}
    h4, c4, _ = _run(SCRIPT_B, dict(args, check=True), "ROWS-B-OK")
    h8, _, _ = _run(SCRIPT_B, dict(args, check=False), "ROWS-B-OK", False)
    assert h4 == h8
    lines = c4[(n, 17, "ref")]
    assert _width(lines) == "4-byte", lines
    assert any("given up" in l and "flagged=0" not in l and "dup=0" in l for l in lines), lines
