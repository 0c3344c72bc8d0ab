"""Times BayesHammer's subclustering (HamClusters.subcluster) over the both-strand 21-mers of the synthetic reads of
tools/kmerdata_perf.py (0.5 % substitutions, host-drawn qualities in [2, 41]): the wall time of the call on the device
path and with BBK_SUBCLUSTER_HOST=1 (the literal algorithm under OpenMP, the threads OMP_NUM_THREADS allows) in the same
library, the kernel times by family from bbk_ctx_profile_get (device events), the cluster-size histogram and the share
of k-mers per size class.  The variable is read at every call, so both paths run in this process; the results of the
two are compared byte for byte.  Prints one JSON line.

    python tools/subcluster_perf.py [--reads 2000000] [--repeats 5]
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

FAMILIES = ("sc_single", "sc_wave", "sc_group", "sc_host_scatter", "sc_finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    k = 21
    ctx = B.Context(0)
    reads = ctx.reads_synth(a.reads, read_len=a.read_len, sub_rate=0.005)
    rng = np.random.default_rng(1)
    qb = rng.integers(2, 42, a.reads * a.read_len, dtype=np.uint8)
    offs = np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(a.read_len)
    quals = ctx.quals(reads, qb, offs)
    del qb
    kset = ctx.count(reads, k, B.BOTH_STRANDS)
    ks = kset.kmer_stats()
    ks.push(reads, quals)
    ks.finish()
    hc = kset.hamming_clusters()
    sizes = hc.sizes()
    n = int(sizes.sum())

    def run(host):
        if host:
            os.environ["BBK_SUBCLUSTER_HOST"] = "1"
        else:
            os.environ.pop("BBK_SUBCLUSTER_HOST", None)
        ctx.synchronize()
        t0 = time.perf_counter()
        sc = hc.subcluster(ks)
        ctx.synchronize()
        return sc, (time.perf_counter() - t0) * 1e3

    out = {"k": k, "reads": a.reads, "read_len": a.read_len, "n": n, "clusters": len(sizes),
           "omp_threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0)}
    edges = [1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 1 << 62]
    out["size_histogram"] = {("%d" % lo if hi == lo + 1 else "%d-%s" % (lo, hi - 1 if hi < 1 << 62 else "")):
                             int(((sizes >= lo) & (sizes < hi)).sum()) for lo, hi in zip(edges, edges[1:])}
    classes = {"size_1": sizes == 1, "size_2_64": (sizes >= 2) & (sizes <= 64), "size_65_256": (sizes >= 65) & (sizes <= 256),
               "above_256": sizes > 256}
    out["kmer_share"] = {name: float(sizes[m].sum()) / n for name, m in classes.items()}
    out["cluster_share"] = {name: float(m.sum()) / len(sizes) for name, m in classes.items()}
    results = {}
    for host in (False, True):
        sc, _ = run(host)  # warm-up: code objects, arena growth
        ctx.profile(True)
        walls, fam = [], {f: [] for f in FAMILIES}
        host_us = []
        for _ in range(a.repeats):
            sc.free()
            ctx.profile_reset()
            sc, wall = run(host)
            walls.append(wall)
            for f in FAMILIES:
                fam[f].append(ctx.profile_get(f)["ms"])
            host_us.append(ctx.profile_get("stat_sc_host_us")["bytes"])
        ctx.profile(False)
        name = "host" if host else "device"
        out[name + "_wall_ms_median"] = float(np.median(walls))
        out[name + "_wall_ms_min"] = min(walls)
        out[name + "_kernel_ms_median"] = {f: float(np.median(v)) for f, v in fam.items()}
        out[name + "_host_algorithm_ms_median"] = float(np.median(host_us)) / 1e3
        out[name + "_host_kmers"] = sc.host_kmers
        r = sc.export()
        results[name] = b"".join(r[f].tobytes() for f in sorted(r))
        out["stats"] = dict(zip(sc.STATS, (int(x) for x in r["stats"])))
        out["solid_kmers"] = int(r["good"].sum())
        sc.free()
    os.environ.pop("BBK_SUBCLUSTER_HOST", None)
    out["same_bytes"] = results["device"] == results["host"]
    out["host_over_device_wall"] = out["host_wall_ms_median"] / out["device_wall_ms_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
