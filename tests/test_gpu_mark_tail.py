"""GPU: the mark-bit scatter tail that k_part_reads_narrow, k_part_view_lt and k_part_lt2 share (msd_mark_tail.h): the
store loop without limits that a tile takes when all its runs fit their slots, the loop with limits and spills
otherwise, the payload instantiation, and k_part_view_lt's bucket-of-a-key from marks.

Every case runs in a fresh process (the switches are read once per process) with BBK_SLOTS_MIN=0 (slot mode at any
size), BBK_POOL_POISON=1 and BBK_VERBOSE=1, and compares the result byte for byte with the oracle in the child (a
switched-off run: with the default run, through the hash).  The
child prints a hash of the result, the "stat_*" counters read through profile_get and the library's verbose lines.
"""
import os
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
mode, k, polya, what, oracle = %(mode)r, %(k)d, %(polya)d, %(what)r, %(oracle)r
rng = np.random.default_rng(9)
if mode == "three":
    reads = ["ACGTTGCAAGTCCGATTAGGCATTAGACCATGACGATTACGGA", "T" * 25 + "G" + "A" * 30, "GATTACAGATTACAGATTACAGATTACA"]
elif mode == "one":
    reads = ["ACGTTGCAAGTCCGATTAGGCATTAGACCATGACGATTACGGA"[:k]]
elif mode == "lowcomplexity":
    g = rng.choice(4, size=%(g)d, p=[0.46, 0.04, 0.04, 0.46])
    starts = rng.integers(0, len(g) - 150, size=%(n)d)
    reads = ["".join("ACGT"[x] for x in g[s:s + 150]) for s in starts]
else:
    reads = synth_reads(%(n)d, read_len=150, genome_len=%(g)d, sub_rate=0.01, seed=5)
    if polya:  # spread among the others, so that many tiles hold a long run of one bin
        step = len(reads) // polya
        for i in range(polya):
            reads.insert(i * (step + 1), "A" * 150)
whole = ctx.reads_from_ascii(reads)
ctx.profile(True)
ctx.profile_reset()
sys.stderr.write("CASE %%s %%d\n" %% (mode, k))
if what == "extindex":
    x = ctx.extindex(whole, k)
    gk, gm = x.export()
    ox = O.ExtIndex(reads, k, 1)
    order = np.lexsort([ox.kmers[:, j] for j in range(ox.kmers.shape[1] - 1, -1, -1)])
    assert np.array_equal(gk, ox.kmers[order]), ("extindex k-mers", len(gk), len(ox.kmers))
    assert np.array_equal(gm, ox.masks[order]), "extindex masks"
    print("ORACLE-EQUAL", len(gk))
    print("HASH", k, len(gk), hashlib.sha256(gk.tobytes() + gm.tobytes()).hexdigest())
    x.free()
else:
    s = ctx.count(whole, k, B.BOTH_STRANDS | B.REFERENCE_ORDER)
    got = s.export(B.ORDER_REFERENCE_BUCKETS16)
    if oracle:
        exp = O.kmercount(reads, k, 16, 2)
        assert np.array_equal(got, exp), (k, len(got), len(exp))
        print("ORACLE-EQUAL", len(exp))
    print("HASH", k, len(got), hashlib.sha256(got.tobytes()).hexdigest())
    s.free()
print("STAT taken", int(ctx.profile_get("stat_late_tag")["launches"]))
print("STAT spilled", int(ctx.profile_get("stat_slot_spilled")["bytes"]))
print("MARK-TAIL-OK")
"""


def _run(mode, k, n=20000, g=200000, polya=0, what="count", late=True, oracle=True):
    env = dict(os.environ, BBK_VERBOSE="1", BBK_POOL_POISON="1", BBK_SLOTS_MIN="0")
    for v in ("BBK_NO_LATE_TAG", "BBK_NO_NARROW_B", "BBK_NO_BUCKET_HANDOFF", "BBK_NO_SLOTS", "BBK_NO_KSLOTS"):
        env.pop(v, None)
    if not late:
        env["BBK_NO_LATE_TAG"] = "1"
    src = SCRIPT % {"root": ROOT, "mode": mode, "k": k, "n": n, "g": g, "polya": polya, "what": what, "oracle": oracle}
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "MARK-TAIL-OK" in r.stdout and ("ORACLE-EQUAL" in r.stdout) == oracle
    out = {"lines": [l for l in r.stderr.splitlines() if "[bbk]" in l]}
    for l in r.stdout.splitlines():
        f = l.split()
        if f[0] == "STAT":
            out[f[1]] = int(f[2])
        elif f[0] == "HASH":
            out["hash"] = l
    print(mode, k, what, "late" if late else "early", {x: out[x] for x in out if x != "lines"})
    for l in out["lines"]:
        print("   ", l)
    return out


# The late-tag route needs 4-byte stage-B records, which the plan grants from ~350 buckets at k = 17, ~1024 at k = 19
# and ~16 k at k = 21 (test_gpu_late_tag.py): 20 000 reads of a 200 kbp genome take it at k = 17 only (measured: "8-byte
# records from level 2 (widest bucket 2^33.5 keys)" at k = 19, 2^37.5 at k = 21).  That input runs at all three k --
# stage A's level 1 and its tail are the same there -- and k = 19, 21 run once more at the smallest sizes of
# test_gpu_late_tag.py at which the route is taken (the default run against the oracle; that file already compares
# those sizes with the switched-off run).
@pytest.mark.parametrize("k,n,g,route", [(17, 20000, 200000, 1), (19, 20000, 200000, 0), (21, 20000, 200000, 0),
                                         (19, 60000, 2000000, 1), (21, 500000, 40000000, 1)])
def test_plain_route_default_against_switched_off(k, n, g, route):
    """(a) the default run and the one without the late tag give the oracle's bytes; the route is taken where it applies"""
    a = _run("plain", k, n, g)
    assert a["taken"] == route, a
    if n == 20000:  # (the switched-off run is held to the oracle through the default run's hash)
        b = _run("plain", k, n, g, late=False, oracle=False)
        assert a["hash"] == b["hash"], "late and early tag differ"
        assert b["taken"] == 0, b


@pytest.mark.parametrize("k", [17, 21])
def test_long_runs_take_the_fast_path(k):
    """(b) the same reads plus 300 reads of 150 A: many tiles hold one bin with hundreds of consecutive staged
    positions (mark words that are all zero)"""
    _run("plain", k, polya=300)


def test_slot_overflow_takes_the_slow_path():
    """(c) 3 000 reads of 150 A among 20 000: 390 k equal records for a level-1 segment slot of about 11 k (mean + 1 % +
    8 192) -- the poly-A segment's sub-slots overflow, their tiles take the loop with limits and spill"""
    a = _run("plain", 21, polya=3000)
    assert a["spilled"] > 0 or any("exact mode" in l for l in a["lines"]), a


def test_payload_instantiation():
    """(d) the extension index of (b)'s input at k = 21: k_part_reads_narrow<true> through the shared tail"""
    _run("plain", 21, polya=300, what="extindex")


def test_late_tag_overflow_reaches_the_stage_b_slow_path():
    """(e) a 92 % A/T genome (test_gpu_late_tag's overflow case): stage B's level-1 sub-slots overflow"""
    a = _run("lowcomplexity", 17, n=40000, g=1000000)
    assert a["taken"] == 1, a


def test_tiles_of_one_record():
    """(f) three reads, and a single read of exactly k bases"""
    _run("three", 21)
    _run("one", 21)
    _run("one", 17)
