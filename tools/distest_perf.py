"""Times the distance-estimation stage (PairInfo.cluster) on the raw paired index of fr pairs cut from a random genome,
over the gbuilder graph of reads of that genome at k = 21: with substitutions in the reads (the junction-rich graph,
--sub 0.003: a bubble or a tip per substitution) or without (the plain graph).  The raw index is filled once; then the
wall time of cluster() on the device path and, as the yardstick, of the library's own host path (BBK_NO_DISTEST_DEVICE:
every pair through the literal search, the same estimation kernel), one warm-up and the median of --repeats each, with
the kernel-family times from bbk_ctx_profile_get (device events) and the share of pairs the device left to the host.
Checks that both paths give the same clusters.  Prints one JSON line.

    python tools/distest_perf.py [--sub 0.003] [--pairs 20000] [--genome 200000] [--repeats 5]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import spades_for_blackbird_amd as B  # noqa: E402
from tests import pairinfo_cases as Cs  # noqa: E402
from tools.pairinfo_perf import cut_pairs  # noqa: E402

FAMILIES = ("distest_walk", "distest_estimate", "scan")
SWITCH = "BBK_NO_DISTEST_DEVICE"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sub", type=float, default=0.003)
    ap.add_argument("--pairs", type=int, default=20_000)
    ap.add_argument("--genome", type=int, default=200_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--raw-filter-threshold", type=int, default=0)
    a = ap.parse_args()
    k, seed = 21, 7
    ctx = B.Context(0)
    cover = ctx.reads_synth(30 * a.genome // a.read_len, read_len=a.read_len, genome_len=a.genome, sub_rate=a.sub,
                            seed_genome=seed, seed_reads=seed + 1)
    tmp = tempfile.TemporaryDirectory()
    gfa = os.path.join(tmp.name, "distest_perf.gfa")
    ctx.unitigs(ctx.extindex(cover, k)).write_gfa(gfa)
    ix = ctx.edgeindex_from_gfa(gfa, k, keep_graph=True)
    first_s, second_s = cut_pairs(Cs.synth_genome(seed, a.genome), a.pairs, a.read_len, seed)
    first, second = ctx.reads_from_ascii(first_s), ctx.reads_from_ascii(second_s)
    pi = ix.pairinfo(0)
    pi.push_estimate(first, second, B.ORIENT_FR)
    st = pi.estimate()
    # a junction-rich graph has no edge long enough to carry both mates: the library's nominal geometry stands in
    mean, dev = (st["mean"], st["deviation"]) if st["ok"] else (400.0, 30.0)
    pi.fill_begin(int(mean), 0, a.raw_filter_threshold)
    pi.push_fill(first, second, B.ORIENT_FR)
    pi.fill_finish()
    prm = dict(insert_size=int(np.floor(mean + 0.5 + 1e-10)), read_length=a.read_len, delta=int(dev), linkage_distance=0,
               max_distance=int(2.0 * dev), filter_threshold=2.0)
    state = {}

    def timed(host):
        if host:
            os.environ[SWITCH] = "1"
        else:
            os.environ.pop(SWITCH, None)
        state[host] = pi.cluster(**prm)  # warm-up: code objects, arena growth, the graph's CSR
        ctx.profile(True)
        walls, fam = [], {f: [] for f in FAMILIES}
        for _ in range(a.repeats):
            ctx.profile_reset()
            ctx.synchronize()
            t0 = time.perf_counter()
            cl = pi.cluster(**prm)
            ctx.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            for f in fam:
                fam[f].append(ctx.profile_get(f)["ms"])
            cl.close()
        ctx.profile(False)
        os.environ.pop(SWITCH, None)
        cl = state[host]
        return {"wall_ms_min": min(walls), "wall_ms_median": float(np.median(walls)),
                "kernel_ms_median": {f: float(np.median(v)) for f, v in fam.items()},
                "pairs": cl.pairs, "host_pairs": cl.host_pairs, "host_share": cl.host_pairs / max(cl.pairs, 1),
                "clusters": len(cl)}

    device, host = timed(False), timed(True)
    same = all(np.array_equal(x, y) for x, y in zip(state[False].export(), state[True].export()))
    out = {"k": k, "sub": a.sub, "pairs_of_reads": a.pairs, "read_len": a.read_len, "genome": a.genome,
           "segments": ix.segments, "raw_points": len(pi.points()[0]), "params": prm, "statistics_ok": bool(st["ok"]),
           "device_path": device, "host_path": host, "same_result": bool(same)}
    print(json.dumps(out))
    tmp.cleanup()
    if not same:
        sys.exit("the device path and the host path disagree")


if __name__ == "__main__":
    main()
