"""The seams of a count step: host waits per call, the fallback paths whose waits moved, the two-array scan.

A flagship-shaped count (odd k <= 21, both strands, final_kmers order, one push) takes five decisions on the host --
the instance count, stage A's level-1 fills, stage A's flags (with the size of stage B), stage B's level-1 fills, stage
B's flags -- and may wait for the stream once for each: "stat_host_waits" counts the waits of the counting path
(bbk_internal.h stream_wait).  The fallback paths (key slots given up, forced spills) may wait more often, and must give
the oracle's result.  The instance count rests on exclusive_scan2_u64 (two arrays, one wait, total behind the output),
checked against numpy.cumsum across one, two and three levels of 4096-item tiles.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import spades_for_blackbird_amd as B
from oracle import oracle as O
from tests.helpers import synth_reads
ctx = B.Context(0)
reads = synth_reads(20000, read_len=150, genome_len=200000, sub_rate=0.01, seed=5)
if %(mode)r == "skew":
    # reads of exactly k bases sharing their first eleven: stage B's 4-byte sort kernel turns their buckets down
    rng = np.random.default_rng(9)
    for k in %(ks)r:
        tails = rng.integers(0, 4, size=(6000, k - 11))
        reads += ["ACGTTGCAAGT" + "".join("ACGT"[x] for x in t) for t in tails]
whole = ctx.reads_from_ascii(reads)
ctx.profile(True)
for k in %(ks)r:
    sys.stderr.write("CASE %%d\n" %% k)
    sys.stderr.flush()
    ctx.profile_reset()
    s = ctx.count(whole, k, B.BOTH_STRANDS | B.REFERENCE_ORDER)
    waits = ctx.profile_get("stat_host_waits")["launches"]
    got = s.export(B.ORDER_REFERENCE_BUCKETS16)
    exp = O.kmercount(reads, k, 16, 2)
    assert np.array_equal(got, exp), (k, len(got), len(exp))
    print("WAITS", k, waits)
    s.free()
print("STEP-OK")
"""


def _run(mode, ks, extra=None):
    env = dict(os.environ, BBK_VERBOSE="1", BBK_POOL_POISON="1", BBK_SLOTS_MIN="0", **(extra or {}))
    for v in ("BBK_NO_BUCKET_HANDOFF", "BBK_DISABLE_MSD", "BBK_NO_SLOTS", "BBK_NO_KSLOTS"):
        env.pop(v, None)
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "mode": mode, "ks": ks}], capture_output=True,
                       text=True, env=env, timeout=1200)
    if r.returncode != 0:
        print(r.stdout[-1500:])
        print(r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-600:]
    assert "STEP-OK" in r.stdout
    waits = {int(l.split()[1]): int(l.split()[2]) for l in r.stdout.splitlines() if l.startswith("WAITS")}
    cases, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.match(r"CASE (\d+)$", line)
        if m:
            cur = int(m.group(1))
            cases[cur] = []
        elif cur is not None and "[bbk]" in line:
            cases[cur].append(line)
    return waits, cases


@pytest.mark.gpu
def test_flagship_shape_waits_once_per_decision():
    """result equal to the oracle (in the child), at most five waits for the call, stage B read the buckets in place"""
    ks = (17, 19, 21)
    waits, cases = _run("small", ks)
    for k in ks:
        print("k=%d: %d host waits" % (k, waits[k]))
    for k in ks:
        lines = cases[k]
        assert any("level 1 read stage A's buckets" in l for l in lines), (k, lines)
        assert any("ordered without histograms" in l for l in lines), (k, lines)
        assert 1 <= waits[k] <= 5, (k, waits[k], lines)


@pytest.mark.gpu
def test_key_slots_given_up_equals_oracle():
    """stage B gives its key slots up after the buckets ran (the decision now comes with the flags)"""
    waits, cases = _run("skew", (17,))
    print("k=17, key slots given up: %d host waits" % waits[17])
    lines = cases[17]
    assert any("level 1 read stage A's buckets" in l for l in lines), lines
    assert any("given up" in l or "records placed, exact mode" in l for l in lines), lines


@pytest.mark.gpu
def test_forced_spills_equal_oracle():
    """stage A's LDS tables give up on crowded buckets: the overflow path runs behind the wait that now also carries
    the size of stage B"""
    waits, cases = _run("small", (19, 21), {"BBK_HASH_MAX_PROBES": "3"})
    over = []
    for k in (19, 21):
        print("k=%d, forced spills: %d host waits" % (k, waits[k]))
        for l in cases[k]:
            m = re.search(r"over_bkt=(\d+)", l)
            if m:
                over.append(int(m.group(1)))
    assert any(o > 0 for o in over), cases


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 4096, 4097, 5000, 3 * 4096 * 4096 // 4 + 13, 4096 * 4096 + 5])
def test_scan2_against_cumsum(n):
    """one level: n <= 4096; two: n <= 4096^2; three above.  In place, entry n receives the total."""
    import torch
    import spades_for_blackbird_amd as B
    L = B.load_library()
    L.bbk_scan2_u64.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.bbk_scan2_u64.restype = C.c_int
    ctx = B.Context(0)
    try:
        rng = np.random.default_rng(n)
        a = rng.integers(0, 1000, size=n + 1, dtype=np.int64)
        b = rng.integers(0, 1 << 33, size=n + 1, dtype=np.int64)  # sums beyond 32 bits
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        torch.cuda.synchronize()
        tot = (C.c_uint64 * 2)()
        rc = L.bbk_scan2_u64(ctx._h, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), n, tot)
        assert rc == 0, L.bbk_last_error()
        for src, dev, t in ((a, da, tot[0]), (b, db, tot[1])):
            exp = np.zeros(n + 1, dtype=np.int64)
            exp[1:] = np.cumsum(src[:n])
            got = dev.cpu().numpy()
            assert t == exp[n], (n, t, exp[n])
            assert np.array_equal(got, exp), (n, np.flatnonzero(got != exp)[:8])
    finally:
        ctx.close()


def test_touched_sources_build_and_host_programs_link():
    """no GPU: every HIP source compiles for gfx950 into the library (the incremental build the entry point runs), no
    kernel uses scratch, the new entry point is exported and the host programs link against it"""
    from spades_for_blackbird_amd import build as b, build_host
    lib = b.build()
    assert os.path.exists(lib)
    for src in ("pool.hip", "context.hip", "scan.hip", "sort.hip", "unique.hip", "msd.hip", "count.hip"):
        obj = os.path.join(b.CSRC, src.replace(".hip", ".o"))
        assert os.path.exists(obj) and os.path.getmtime(obj) >= os.path.getmtime(os.path.join(b.CSRC, src)), src
    res = b.check_resources()
    if res is not None:
        names = " ".join(r[1] for r in res)
        for kern in ("k_scan_reduce", "k_scan_apply", "k_bucket_init", "k_tile_reads"):
            assert kern in names, kern
    assert hasattr(C.CDLL(lib), "bbk_scan2_u64")
    for exe in build_host.build():
        assert os.path.exists(exe), exe
