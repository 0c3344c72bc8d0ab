"""GPU: stage B with 4-byte records after level 1 (msd_stage_b.h "narrow stage B", k_bucket_base / k_bucket_dist_nb).

The ordering pass of the both-strand set takes the key slots; when no level-2 bucket spans more than 2^32 keys only the
keys' low words travel from level 2 on and the sort kernel widens them with the bucket's smallest key.  Every case is
run twice, in fresh processes (the switches are read once per process): as it is and with BBK_NO_NARROW_B=1 (8-byte
records throughout).  Both must give the same bytes, and the small cases must also equal the oracle.  The BBK_VERBOSE
line of every call says which path ran.  Device memory is poisoned, so a slot or bucket read past what was written
shows up as garbage keys.
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
mode = %(mode)r
if mode == "large":
    whole = ctx.reads_synth(%(n)d, read_len=150, genome_len=%(g)d)
    reads = None
else:
    reads = synth_reads(%(n)d, read_len=150, genome_len=%(g)d, sub_rate=0.01, seed=5)
    if mode == "skew":
        # reads of exactly k bases sharing their first eleven: thousands of distinct keys inside 2^(2k - 22)-key ranges,
        # which crowd one distribution bin of their buckets -- the sort kernel turns those buckets down
        rng = np.random.default_rng(9)
        for k in %(ks)r:
            tails = rng.integers(0, 4, size=(6000, k - 11))
            reads += ["ACGTTGCAAGT" + "".join("ACGT"[x] for x in t) for t in tails]
    whole = ctx.reads_from_ascii(reads)
for k in %(ks)r:
    for flags, name in ((B.BOTH_STRANDS | B.REFERENCE_ORDER, "ref"), (B.BOTH_STRANDS, "plain")):
        sys.stderr.write("CASE %%d %%s\n" %% (k, name))
        sys.stderr.flush()
        s = ctx.count(whole, k, flags)
        got = s.export(B.ORDER_REFERENCE_BUCKETS16 if name == "ref" else B.ORDER_SORTED)
        runs, eq, _ = s.verify_order()
        assert eq == 0, (k, name, "equal neighbours", eq)
        if name == "plain":
            assert runs == 1, (k, name, "not ascending", runs)
        if reads is not None:
            exp = O.kmercount(reads, k, 16, 2)
            if name == "plain":
                exp = np.sort(exp[:, 0]).reshape(-1, 1)
            assert np.array_equal(got, exp), (k, name, len(got), len(exp))
        print("HASH", k, name, len(got), hashlib.sha256(got.tobytes()).hexdigest())
        s.free()
print("NARROW-B-OK")
"""


def _run(mode, n, g, ks, narrow, extra=None):
    env = dict(os.environ, BBK_VERBOSE="1", BBK_POOL_POISON="1", **(extra or {}))
    env.pop("BBK_NO_NARROW_B", None)
    if not narrow:
        env["BBK_NO_NARROW_B"] = "1"
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "mode": mode, "n": n, "g": g, "ks": ks}],
                       capture_output=True, text=True, env=env, timeout=1200)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "NARROW-B-OK" in r.stdout
    hashes = [l for l in r.stdout.splitlines() if l.startswith("HASH")]
    return hashes, _cases(r.stderr)


def _cases(err):
    """{(k, name): [verbose lines of that call]}"""
    out, cur = {}, None
    for line in err.splitlines():
        m = re.match(r"CASE (\d+) (\w+)$", line)
        if m:
            cur = (int(m.group(1)), m.group(2))
            out[cur] = []
        elif cur is not None and "[bbk]" in line:
            out[cur].append(line)
    return out


def _path(lines):
    """record width of the key-slot attempt of a call: "4-byte", "8-byte" or None (no key slots)"""
    for l in lines:
        m = re.search(r"msd key slots: (\d)-byte records", l)
        if m:
            return m.group(1) + "-byte"
    return None


def _both(mode, n, g, ks, extra=None):
    h4, c4 = _run(mode, n, g, ks, True, extra)
    h8, c8 = _run(mode, n, g, ks, False, extra)
    assert h4 == h8, "4-byte and 8-byte stage B differ"
    for case, lines in c8.items():
        assert _path(lines) in ("8-byte", None), (case, lines)
    return c4


def test_narrow_stage_b_small_k():
    """k = 15, 17, 19 on ~1.4 M both-strand records (~350 buckets) with the key slots forced on: final_kmers order (tagged
    (k+2)-mers) and ascending order (plain k-mers) take the 4-byte records wherever the buckets span at most 2^32 keys.
    Tagged k = 19 needs ~1024 buckets for that, so it takes the 8-byte records: the fallback, equally exact."""
    cases = _both("small", 20000, 200000, (15, 17, 19), {"BBK_SLOTS_MIN": "0"})
    for case in ((15, "ref"), (15, "plain"), (17, "ref"), (17, "plain"), (19, "plain")):
        assert _path(cases[case]) == "4-byte", (case, cases[case])
        assert any("ordered without histograms" in l for l in cases[case]), (case, cases[case])
    assert _path(cases[(19, "ref")]) == "8-byte", cases[(19, "ref")]


def test_narrow_stage_b_span_check_fails_at_small_k21():
    """tagged k = 21 spans 2^46 keys: a bucket holds at most 2^32 of them only from ~16 k buckets (~64 M records) on; at
    this size the check fails and the 8-byte path runs"""
    cases = _both("small", 20000, 200000, (21,), {"BBK_SLOTS_MIN": "0"})
    assert _path(cases[(21, "ref")]) == "8-byte", cases[(21, "ref")]
    assert any("ordered without histograms" in l for l in cases[(21, "ref")])


def test_narrow_stage_b_give_up_to_exact_mode():
    """buckets the 4-byte sort kernel turns down (a crowded distribution bin) send the call back to the exact mode"""
    cases = _both("skew", 20000, 200000, (17,), {"BBK_SLOTS_MIN": "0"})
    lines = cases[(17, "ref")]
    assert _path(lines) == "4-byte", lines
    assert any("given up" in l and "flagged=0" not in l for l in lines), lines


def test_narrow_stage_b_k21_at_scale():
    """the flagship k at the bench's 50x coverage: 2.5 M reads, ~90 M both-strand records (~90 buckets per segment, 64
    needed) -- the span check passes, with the default slot threshold"""
    cases = _both("large", 2_500_000, 7_500_000, (21,))
    for name in ("ref", "plain"):
        assert _path(cases[(21, name)]) == "4-byte", cases[(21, name)]
        assert any("ordered without histograms" in l for l in cases[(21, name)])
