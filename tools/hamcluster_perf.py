"""Times the Hamming-graph clustering (KMerSet.hamming_clusters, tau = 1) of the both-strand 21-mers of synthetic reads
with 0.5 % substitutions: kernel-family times from bbk_ctx_profile_get (device events), the wall time of the call, and
the wall time of the both-strand count of the same reads as the yardstick.  Prints one JSON line.

    python tools/hamcluster_perf.py [--reads 2000000] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import spades_for_blackbird_amd as B  # noqa: E402

# rc index, block scan (the hooking runs inside it), pointer-jumping rounds, sizes + compaction + listing kernels; the
# listing's sort runs in the LSD families
FAMILIES = ("hc_rcidx", "hc_scan", "hc_jump", "hc_list", "hist", "scan", "scatter")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    k = 21
    ctx = B.Context(0)
    reads = ctx.reads_synth(a.reads, read_len=a.read_len, sub_rate=0.005)

    def timed(fn, families=()):
        out = fn()  # warm-up: code objects, arena growth
        ctx.profile(True)
        walls, fam, stats = [], {f: [] for f in families}, {}
        for _ in range(a.repeats):
            del out
            ctx.profile_reset()
            ctx.synchronize()
            t0 = time.perf_counter()
            out = fn()
            ctx.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            for f in families:
                fam[f].append(ctx.profile_get(f)["ms"])
            for s in ("stat_hc_largest_block", "stat_hc_rounds"):
                stats[s] = int(ctx.profile_get(s)["bytes"])
        ctx.profile(False)
        return out, {"wall_ms_min": min(walls), "wall_ms_median": float(np.median(walls)),
                     "kernel_ms_median": {f: float(np.median(v)) for f, v in fam.items()}}, stats

    kset, count_t, _ = timed(lambda: ctx.count(reads, k, B.BOTH_STRANDS))
    h, clust_t, stats = timed(lambda: kset.hamming_clusters(), FAMILIES)
    sizes = h.sizes()
    out = {"k": k, "reads": a.reads, "read_len": a.read_len, "n": len(kset), "clusters": len(h),
           "largest_cluster": int(sizes.max()) if len(sizes) else 0, "largest_block": stats["stat_hc_largest_block"],
           "hooking_rounds": stats["stat_hc_rounds"], "replayed": h.replayed, "clustering": clust_t,
           "count_both_strands": {"wall_ms_min": count_t["wall_ms_min"], "wall_ms_median": count_t["wall_ms_median"]}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
