"""GPU: tagged stage B with 4-byte records from level 1 and the tag taken at level 2 (msd_stage_b.h "late tag",
k_part_view_lt / k_part_lt2 / k_bucket_base_lt).

The route applies to the flagship shape (both strands, final_kmers order, stage A's buckets handed over in place) at
17 <= k <= 21 when the call is large enough for 4-byte stage-B records at all; BBK_NO_LATE_TAG=1 switches it off.  Every
case runs in fresh processes (the switches are read once per process), with the device pool poisoned.  The child prints a
hash of every result and the "stat_late_tag" counters read through profile_get, so a case cannot pass on the fallback
unnoticed.  The sizes: 4-byte stage-B records need buckets of at most 2^32 tagged keys, i.e. ~350 buckets at k = 17,
~1024 at k = 19 and ~16 k (70 M both-strand records) at k = 21.
"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("BBK_DISABLE_MSD")), reason="tests of the MSD path's modes")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %(root)r)
import spades_for_blackbird_amd as B
from oracle import oracle as O
from tests.helpers import synth_reads
ctx = B.Context(0)
mode, k, oracle = %(mode)r, %(k)d, %(oracle)r
rng = np.random.default_rng(9)
if mode == "tiny":
    reads = ["T" * 40, "ACGTTGCAAGTCCGATTAGGCATTAGACCATGACGATTACGGA", "T" * 25 + "G" + "A" * 30]
elif mode == "lowcomplexity":
    # 92 %% A/T: the five bases of a k-mer that name its key-prefix segment are far from uniform
    g = rng.choice(4, size=%(g)d, p=[0.46, 0.04, 0.04, 0.46])
    starts = rng.integers(0, len(g) - 150, size=%(n)d)
    reads = ["".join("ACGT"[x] for x in g[s:s + 150]) for s in starts]
else:
    reads = synth_reads(%(n)d, read_len=150, genome_len=%(g)d, sub_rate=0.01, seed=5)
    if mode == "crowded":
        # reads of exactly k bases sharing their first eleven: the sort kernel turns their buckets down (a crowded
        # distribution bin) after level 1 has released stage A's buckets
        tails = rng.integers(0, 4, size=(6000, k - 11))
        reads += ["ACGTTGCAAGT" + "".join("ACGT"[x] for x in t) for t in tails]
    if mode == "allT":
        reads += ["T" * 60, "A" * 45 + "C" + "T" * 50, "G" + "T" * (k + 3)]
whole = ctx.reads_from_ascii(reads)
ctx.profile(True)
ctx.profile_reset()
sys.stderr.write("CASE %%d\n" %% k)
s = ctx.count(whole, k, B.BOTH_STRANDS | B.REFERENCE_ORDER)
got = s.export(B.ORDER_REFERENCE_BUCKETS16)
print("STAT taken", ctx.profile_get("stat_late_tag")["launches"])
print("STAT recanon", ctx.profile_get("stat_late_tag_recanon")["launches"])
runs, eq, _ = s.verify_order()
assert eq == 0, ("equal neighbours", eq)
if oracle:
    exp = O.kmercount(reads, k, 16, 2)
    assert np.array_equal(got, exp), (k, len(got), len(exp))
    print("ORACLE-EQUAL", len(exp))
print("HASH", k, len(got), hashlib.sha256(got.tobytes()).hexdigest())
s.free()
print("LATE-TAG-OK")
"""


def _run(mode, k, n=20000, g=200000, late=True, oracle=True, extra=None):
    env = dict(os.environ, BBK_VERBOSE="1", BBK_POOL_POISON="1", BBK_SLOTS_MIN="0", **(extra or {}))
    for v in ("BBK_NO_LATE_TAG", "BBK_NO_NARROW_B", "BBK_NO_BUCKET_HANDOFF", "BBK_NO_SLOTS", "BBK_NO_KSLOTS"):
        env.pop(v, None)
    if not late:
        env["BBK_NO_LATE_TAG"] = "1"
    src = SCRIPT % {"root": ROOT, "mode": mode, "k": k, "n": n, "g": g, "oracle": oracle}
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, env=env, timeout=1500)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "LATE-TAG-OK" in r.stdout
    out = {"lines": [l for l in r.stderr.splitlines() if "[bbk]" in l]}
    for l in r.stdout.splitlines():
        f = l.split()
        if f[0] == "STAT":
            out[f[1]] = int(f[2])
        elif f[0] == "HASH":
            out["hash"] = l
        elif f[0] == "ORACLE-EQUAL":
            out["oracle"] = int(f[1])
    print(mode, k, "late" if late else "early", {x: out[x] for x in out if x != "lines"})
    return out


def _ab(mode, k, n=20000, g=200000):
    """default (checked against the oracle in the child) and switched off: same bytes, the route only in the former"""
    a = _run(mode, k, n, g, late=True, oracle=True)
    b = _run(mode, k, n, g, late=False, oracle=False)
    assert "oracle" in a
    assert a["hash"] == b["hash"], "late and early tag differ"
    assert b["taken"] == 0 and b["recanon"] == 0, b
    return a


@pytest.mark.parametrize("k,n,g", [(17, 20000, 200000), (19, 60000, 2000000), (21, 500000, 40000000)])
def test_late_tag_equals_oracle_and_early_tag(k, n, g):
    """k = 17, 19, 21 at sizes where 4-byte stage-B records apply: the route is taken, holds (no histograms), and gives
    the oracle's bytes and the bytes of the switched-off run"""
    a = _ab("plain", k, n, g)
    assert a["taken"] == 1, a
    assert any("tag taken at level 2" in l for l in a["lines"]), a["lines"]
    assert any("ordered without histograms" in l for l in a["lines"]), a["lines"]
    assert a["recanon"] == 0, a


@pytest.mark.parametrize("k", [22, 31])
def test_other_k_do_not_take_the_route(k):
    a = _ab("plain", k)
    assert a["taken"] == 0, a
    assert not any("tag taken at level 2" in l for l in a["lines"]), a["lines"]


def test_all_t_kmer_and_tiny_input():
    """the all-T k-mer (lo = all ones, the last segment) inside a call that takes the route; a few reads (no slot mode)"""
    a = _ab("allT", 17)
    assert a["taken"] == 1, a
    t = _ab("tiny", 17)
    assert t["taken"] == 0, t


def test_low_complexity_overflows_segments_and_falls_back():
    """a 92 % A/T genome: the key-prefix segments overflow their slots, the exact mode gives the oracle's result.

    The size that overflows: each of the 32 segments named by five A/T bases takes 0.46^5 = 2.06 % of the both-strand
    set, an eighth of it per (segment, XCD) sub-slot, and a sub-slot holds N / 8192 * 1.06 + 2048 records.  The fixed
    2048 is what a small call hides behind: 0.0206 N / 8 > N / 8192 * 1.06 + 2048 needs N > 0.84 M.  A 1 M-base genome
    at 5x k-mer coverage gives N ~ 1.9 M both-strand k-mers: ~4.9 k records for a sub-slot of ~2.3 k."""
    a = _ab("lowcomplexity", 17, n=40000, g=1000000)
    assert a["taken"] == 1, a
    assert any("segments overflow, exact mode" in l or "records placed, exact mode" in l or "given up" in l
               for l in a["lines"]), a["lines"]
    assert not any("ordered without histograms" in l for l in a["lines"]), a["lines"]


def test_give_up_after_hand_off_rebuilds_from_4_byte_records():
    """buckets the sort kernel turns down after level 1 released stage A's buckets: the canonical keys come back from
    the 4-byte level-1 records (k_view_recanon_lt), then the exact mode"""
    a = _ab("crowded", 17)
    assert a["taken"] == 1, a
    assert a["recanon"] == 1, (a, a["lines"])
    assert any("given up" in l or "records placed, exact mode" in l for l in a["lines"]), a["lines"]
