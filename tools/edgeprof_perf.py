"""Times the graph-mapping stage (csrc/edgeprof.hip): the edge index of a unitig graph, the edge profile of a read set
(bbk_profiles_push_reads) and its mapping paths (bbk_edgeindex_map_paths), at k = 21 and k = 55.  The reads are
synthetic 150-base reads and the graph is the unitig graph of those reads.  Kernel-family times come from
bbk_ctx_profile_get (device events), wall times are taken around calls that end in a synchronise; map_paths' wall time
includes the export of the ranges to the host.  Prints one JSON line.

    python tools/edgeprof_perf.py [--reads 1000000] [--repeats 5] [--k 21 55]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--k", type=int, nargs="+", default=[21, 55])
    a = ap.parse_args()
    ctx = B.Context(0)
    reads = ctx.reads_synth(a.reads, read_len=150, sub_rate=0.003)

    def timed(fn, families):
        fn()  # warm-up: code objects, arena growth
        ctx.profile(True)
        walls, fam = [], {f: [] for f in families}
        for _ in range(a.repeats):
            ctx.profile_reset()
            ctx.synchronize()
            t0 = time.perf_counter()
            out = fn()
            ctx.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            for f in families:
                fam[f].append(ctx.profile_get(f)["ms"])
        ctx.profile(False)
        return out, {"wall_ms_min": min(walls), "wall_ms_median": float(np.median(walls)),
                     "kernel_ms_median": {f: float(np.median(v)) for f, v in fam.items()}}

    out = {"reads": a.reads, "read_len": 150, "repeats": a.repeats, "k": {}}
    for k in a.k:
        unitigs = ctx.unitigs(ctx.extindex(reads, k))
        ix, index_t = timed(lambda: ctx.edgeindex_from_unitigs(unitigs), ("edgeindex",))
        prof = ix.profiles(1)
        _, push_t = timed(lambda: prof.push(0, reads), ("edgeprof_map",))
        (off, rec), paths_t = timed(lambda: ix.map_paths(reads), ("gmap_count", "gmap_write"))
        out["k"][str(k)] = {"segments": ix.segments, "indexed": len(ix), "ranges": len(rec),
                            "raw_sum": int(prof.raw().sum()) // (a.repeats + 1),  # one push of the reads
                            "index": index_t, "push_reads": push_t, "map_paths": paths_t}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
