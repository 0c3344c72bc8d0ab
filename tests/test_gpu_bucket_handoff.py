"""GPU: stage B's level 1 reading stage A's buckets in place (msd.h BucketView, msd_stage_b.h k_part_view).

A single-batch both-strand count at odd k with 8-byte keys leaves stage A's distinct set in its level-2 slots; the key
slots of stage B read it there, and nothing else ever sees it: every other consumer materialises the dense array
first.  Every case runs in fresh processes (the switch is read once per process), as it is and with
BBK_NO_BUCKET_HANDOFF=1 (the dense hand-off).  Both must give the same bytes, the small cases must equal the oracle,
and the BBK_VERBOSE lines must show which hand-off ran.  Device memory is poisoned, so a slot read past what stage A
wrote shows up as garbage keys.
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
if mode == "empty":
    reads = ["ACGTACGTAC"] * 5  # shorter than k: no k-mer at all
else:
    reads = synth_reads(%(n)d, read_len=150, genome_len=%(g)d, sub_rate=0.01, seed=5)
if mode == "skew":
    # reads of exactly k bases sharing their first eleven: the 4-byte sort kernel of stage B turns their buckets down
    rng = np.random.default_rng(9)
    for k in %(ks)r:
        tails = rng.integers(0, 4, size=(6000, k - 11))
        reads += ["ACGTTGCAAGT" + "".join("ACGT"[x] for x in t) for t in tails]
whole = ctx.reads_from_ascii(reads)
for k in %(ks)r:
    for flags, name in ((B.BOTH_STRANDS | B.REFERENCE_ORDER, "ref"), (B.BOTH_STRANDS, "plain")):
        sys.stderr.write("CASE %%d %%s\n" %% (k, name))
        sys.stderr.flush()
        if mode == "stream":
            c = ctx.counter(k, flags)
            step = (len(reads) + 2) // 3
            for a in range(0, len(reads), step):
                c.push_ascii(reads[a:a + step])
            s = c.finish()
        else:
            s = ctx.count(whole, k, flags)
        got = s.export(B.ORDER_REFERENCE_BUCKETS16 if name == "ref" else B.ORDER_SORTED)
        if mode == "empty":
            assert len(got) == 0, (k, name, len(got))
            print("HASH", k, name, 0)
            s.free()
            continue
        exp = O.kmercount(reads, k, 16, 2)
        if name == "plain":
            exp = np.sort(exp[:, 0]).reshape(-1, 1)
        assert np.array_equal(got, exp), (k, name, len(got), len(exp))
        print("HASH", k, name, len(got), hashlib.sha256(got.tobytes()).hexdigest())
        s.free()
print("HANDOFF-OK")
"""


def _run(mode, n, g, ks, handoff, extra=None):
    env = dict(os.environ, BBK_VERBOSE="1", BBK_POOL_POISON="1", BBK_SLOTS_MIN="0", **(extra or {}))
    env.pop("BBK_NO_BUCKET_HANDOFF", None)
    if not handoff:
        env["BBK_NO_BUCKET_HANDOFF"] = "1"
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "mode": mode, "n": n, "g": g, "ks": ks}],
                       capture_output=True, text=True, env=env, timeout=1200)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "HANDOFF-OK" in r.stdout
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


def _handoff(lines):
    """what stage A handed over: "bucket view", "dense array" or None (not asked)"""
    for l in lines:
        m = re.search(r"msd hand-off to stage B: (bucket view|dense array)", l)
        if m:
            return m.group(1)
    return None


def _read_in_place(lines):
    """(buckets' keys, overflow keys) of a level 1 that read the view, else None"""
    for l in lines:
        m = re.search(r"level 1 read stage A's buckets \((\d+) \+ (\d+) keys\)", l)
        if m:
            return int(m.group(1)), int(m.group(2))
    return None


def _both(mode, n, g, ks, extra=None):
    hv, cv = _run(mode, n, g, ks, True, extra)
    hd, cd = _run(mode, n, g, ks, False, extra)
    assert hv == hd, "bucket view and dense hand-off differ"
    for case, lines in cd.items():
        assert _handoff(lines) in ("dense array", None), (case, lines)
        assert _read_in_place(lines) is None, (case, lines)
    return cv


def test_handoff_k17_to_21():
    """odd k reads the buckets in place, in final_kmers order (tagged) and ascending; even k is never offered a view
    (no key slots without a distinct expanded set)"""
    cases = _both("small", 20000, 200000, (17, 18, 19, 20, 21))
    for k in (17, 19, 21):
        for name in ("ref", "plain"):
            lines = cases[(k, name)]
            assert _handoff(lines) == "bucket view", (k, name, lines)
            assert _read_in_place(lines) is not None, (k, name, lines)
    for k in (18, 20):
        for name in ("ref", "plain"):
            assert _handoff(cases[(k, name)]) is None, (k, name, cases[(k, name)])


def test_handoff_overflow_tail():
    """stage A's LDS tables give up on crowded buckets: their keys come from the overflow path as 8-byte keys and are
    scattered by a second launch into the same level-1 slots"""
    cases = _both("small", 20000, 200000, (19, 21), {"BBK_HASH_MAX_PROBES": "3"})
    tails = []
    for case, lines in cases.items():
        if _handoff(lines) == "bucket view":  # (a pass whose overflow outweighs half its input leaves the narrow mode)
            assert _read_in_place(lines) is not None, (case, lines)
            tails.append(_read_in_place(lines))
    assert any(t[1] > 0 for t in tails), tails


def test_handoff_key_slots_give_up():
    """stage B gives its key slots up after level 1 has released the buckets: the canonical keys are rebuilt from the
    level-1 records and the exact mode finishes"""
    cases = _both("skew", 20000, 200000, (17,))
    lines = cases[(17, "ref")]
    assert _read_in_place(lines) is not None, lines
    assert any("given up" in l and "flagged=0" not in l for l in lines), lines


def test_handoff_streaming_takes_dense():
    """several pushes: the first batch's view is materialised when the second arrives"""
    cases = _both("stream", 20000, 200000, (21,))
    for name in ("ref", "plain"):
        assert _read_in_place(cases[(21, name)]) is None, cases[(21, name)]


def test_handoff_empty_input():
    _both("empty", 0, 0, (21,))
