"""GPU: stage A's level 2 (k_part_narrow2) on the mark-bit tail of msd_mark_tail.h in its RANKED form, with the 16-byte
loads of its tile rows (tile_rows4, msd_narrow_a.h).

Every case runs in a fresh process with BBK_SLOTS_MIN=0, BBK_POOL_POISON=1 and BBK_VERBOSE=1 and is compared with the
oracle in the child; the child scripts are those of test_gpu_bucket_rows.py and test_gpu_mark_tail.py.

A level-2 tile is what one level-1 sub-slot holds, cut into pieces of 12 288 records; a lane loads it as three groups
of four records, group r covering records r * 4096 .. r * 4096 + 4095.  The library's verbose line "msd level-2 tiles"
says how many tiles of the call were whole and how many last tiles of a sub-slot reached one, two and three groups,
and the tests assert on it:

- CANONICAL | UNSORTED at k = 17, 19, 21 over 3 000, 8 000 and 38 000 reads of 150 bp (0.4 M, 1 M and 5 M records).
  On a device of 8 XCDs level 1 fills 8192 sub-slots, so these are tiles of about 50, 130 and 620 records: all of one
  group, with every remainder mod 4 among the thousands of them (the last group of four of a tile is partial in all
  three ways and whole).
- the same at k = 17 and 21 with BBK_XCD_SLOTS=0 (1024 sub-slots, one per segment) over 55 000, 80 000 and 100 000
  reads (7 M, 10 M and 13 M records): about 7 000, 10 000 and 12 700 records per sub-slot, so last tiles of two and of
  three groups, whole tiles, and behind a whole tile a tile that begins at record 12 288 of its sub-slot.

Stage B, the 16-byte row loads of k_bucket_dist_nb (its first eight records per lane as two groups of four, records
0 .. 2047 and 2048 .. 4095 of the bucket, then single rows): the read counts of test_gpu_bucket_rows.py at k = 15 and
17 in both orders, byte-equal to the oracle and to the BBK_NO_NARROW_B=1 run, no duplicate reported.  That file's plan
(plan_fills, the ascending order's buckets) gives every bucket's fill: fills with every remainder mod 4, fills that
end in the second group and fills that reach the single rows must occur; buckets that end in the first group are the
tagged order's at k = 17 (a few dozen records each, by the mean of the call's verbose line).
"""
import os
import re
import subprocess
import sys

import pytest

from tests.test_gpu_bucket_rows import GENOME, SCRIPT_A, SCRIPT_B, SWEEP, _cases, _ordered, _width
from tests.test_gpu_mark_tail import _run as _run_tail

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("BBK_DISABLE_MSD")), reason="tests of the MSD path's modes")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (that file adds its reads that begin with T x 16 to the second size of its list: here, to one size; and it walks
# k = 17, 19, 21: here, the k of the case)
assert SCRIPT_A.count("if n == %(ns)r[1]:") == 1 and SCRIPT_A.count("for k in (17, 19, 21):") == 1
SCRIPT_A_KS = SCRIPT_A.replace("if n == %(ns)r[1]:", "if n == 8000:").replace("for k in (17, 19, 21):", "for k in %(ks)r:")


def _tiles(lines):
    """(whole tiles, last tiles of one / two / three groups, largest sub-slot) of a call's verbose lines"""
    for l in lines:
        m = re.search(r"msd level-2 tiles \(narrow records\): whole=(\d+) groups1=(\d+) groups2=(\d+) groups3=(\d+) "
                      r"largest_sub_slot=(\d+)", l)
        if m:
            return tuple(int(x) for x in m.groups())
    return None


def _run_a(n, ks, xcd_slots):
    env = dict(os.environ, BBK_VERBOSE="1", BBK_POOL_POISON="1", BBK_SLOTS_MIN="0")
    env.pop("BBK_XCD_SLOTS", None)
    if not xcd_slots:
        env["BBK_XCD_SLOTS"] = "0"
    src = SCRIPT_A_KS % {"root": ROOT, "g": GENOME, "ns": [n], "ks": tuple(ks)}
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ROWS-A-OK" in r.stdout
    cases = _cases(r.stderr)
    out = {}
    for k in ks:
        lines = cases[(n, k, "canon")]
        assert any("msd slots (narrow records)" in l for l in lines), (n, k, lines)
        out[k] = _tiles(lines)
        assert out[k] is not None, (n, k, lines)
        print(n, k, "xcd_slots" if xcd_slots else "segment slots", "whole, groups 1 / 2 / 3, largest sub-slot:", out[k])
    return out


@pytest.mark.parametrize("n", [3000, 8000, 38000])
def test_stage_a_level2_against_the_oracle(n):
    """CANONICAL | UNSORTED at k = 17, 19, 21 as a sorted set against the oracle's canonical set, on the narrow route:
    thousands of tiles of one group of four, none empty of records"""
    for k, (whole, g1, g2, g3, largest) in _run_a(n, (17, 19, 21), True).items():
        assert g1 >= 1024 and largest < 12288, (n, k, whole, g1, g2, g3, largest)


@pytest.mark.parametrize("n,want", [(55000, "two"), (80000, "three"), (100000, "whole")])
def test_stage_a_level2_tiles_of_two_and_three_groups_and_whole_tiles(n, want):
    """one sub-slot per segment (BBK_XCD_SLOTS=0), sub-slots of about 7 000, 10 000 and 12 700 records: the second and
    the third group of four of a lane hold records, the re-read of the last group happens in a later group, and a
    sub-slot above 12 288 records has a whole tile and a tile that begins at a multiple of 12 288"""
    for k, (whole, g1, g2, g3, largest) in _run_a(n, (17, 21), False).items():
        if want == "two":
            assert g2 >= 100 and largest > 4096, (n, k, whole, g1, g2, g3, largest)
        elif want == "three":
            assert g3 >= 100 and largest > 8192, (n, k, whole, g1, g2, g3, largest)
        else:
            # a whole tile, with a short tile behind it that begins at record 12 288 of its sub-slot
            assert whole >= 100 and g1 >= 100 and largest > 12288, (n, k, whole, g1, g2, g3, largest)


@pytest.mark.parametrize("k,polya,level2_alone", [(21, 3000, False), (17, 80, True)])
def test_level2_overflow_takes_the_loop_with_limits_and_spills(k, polya, level2_alone):
    """poly-A reads spread among 20 000 others, as test_gpu_mark_tail.py spreads them: 3 000 of them (390 k equal
    records) overflow their level-1 segment; 80 (10 k equal records, with the segment's own 2.6 k below its capacity of
    19 k) pass level 1 and overflow the one level-2 bucket slot of their segment (8 192 records): the level-2 tiles that
    hold them take the loop with limits and the spill loop.  Spills counted, result equal to the oracle."""
    a = _run_tail("plain", k, polya=polya)
    assert a["spilled"] > 0, a
    if level2_alone:
        line = [l for l in a["lines"] if "msd slots (narrow records)" in l]
        assert line and "over_seg=0" in line[0] and "over_bkt=0" not in line[0], a


def test_extension_index_through_level2():
    """k_part_narrow2<true> (payload: the mask byte) on the shared tail, 8 000 reads at k = 21 against the oracle, on
    the narrow route (its level-2 tiles are listed)"""
    a = _run_tail("plain", 21, n=8000, what="extindex")
    assert any("msd slots (narrow records)" in l for l in a["lines"]), a
    assert _tiles(a["lines"]) is not None, a


_FILLS_LINE = '                    print("FILLS"'
_SHAPES = ('                    live = f[f > 0]\n'
           '                    print("SHAPES", n, k, *(int(((live & 3) == a).sum()) for a in range(4)),\n'
           '                          int((live <= 2048).sum()), int(((live > 2048) & (live <= 4096)).sum()), int((live > 4096).sum()))\n')
assert SCRIPT_B.count(_FILLS_LINE) == 1
SCRIPT_B_SHAPES = SCRIPT_B.replace(_FILLS_LINE, _SHAPES + _FILLS_LINE)


def _run_b(narrow):
    env = dict(os.environ, BBK_VERBOSE="1", BBK_POOL_POISON="1", BBK_SLOTS_MIN="0")
    env.pop("BBK_NO_NARROW_B", None)
    if not narrow:
        env["BBK_NO_NARROW_B"] = "1"
    args = {"ns": SWEEP, "ks": (15, 17), "skew": False, "hot": 0, "check": narrow, "root": ROOT, "g": GENOME}
    r = subprocess.run([sys.executable, "-c", SCRIPT_B_SHAPES % args], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ROWS-B-OK" in r.stdout
    shapes = {}
    for l in r.stdout.splitlines():
        if l.startswith("SHAPES"):
            v = [int(x) for x in l.split()[1:]]
            shapes[(v[0], v[1])] = v[2:]
    return [l for l in r.stdout.splitlines() if l.startswith("HASH")], _cases(r.stderr), shapes


@pytest.fixture(scope="module")
def stage_b():
    return _run_b(True), _run_b(False)


@pytest.mark.parametrize("n", SWEEP)
def test_sort_kernel_wide_loads_against_the_oracle_and_the_8_byte_route(stage_b, n):
    """oracle-equal (asserted inside the run), byte-equal to the BBK_NO_NARROW_B=1 run, on the 4-byte route, no bucket
    turned down and no duplicate reported (either would give the key slots up)"""
    (h4, c4, _), (h8, c8, _) = stage_b
    mine = [l for l in h4 if l.split()[1] == str(n)]
    assert len(mine) == 4 and mine == [l for l in h8 if l.split()[1] == str(n)]
    for k in (15, 17):
        for name in ("ref", "plain"):
            lines = c4[(n, k, name)]
            assert _width(lines) == "4-byte", (n, k, name, lines)
            assert not any("given up" in l or "withdrawn" in l for l in lines), lines
            assert _ordered(lines) is not None, lines
            assert _width(c8[(n, k, name)]) in ("8-byte", None), c8[(n, k, name)]


def test_sort_kernel_bucket_shapes_of_the_sweep(stage_b):
    """from the plan, over the sweep: fills with every remainder mod 4 (the last group of four of a bucket partial in
    all three ways and whole), fills that end in the second group of four and fills that reach the single rows; and
    buckets that end in the first group, by the mean fill of the tagged order at k = 17"""
    (_, c4, shapes), _ = stage_b
    assert len(shapes) == 2 * len(SWEEP), shapes
    tot = [sum(v[i] for v in shapes.values()) for i in range(7)]
    print("fills mod 4 = 0, 1, 2, 3; fills <= 2048, <= 4096, above:", tot)
    assert all(t > 0 for t in tot[:4]) and tot[5] > 0 and tot[6] > 0, tot
    means = [N / nb for N, nb in (_ordered(lines) for lines in c4.values())]
    assert min(means) < 512, sorted(means)
