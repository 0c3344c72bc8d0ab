"""Times the k-mer profile join and the contig abundances at the skewed-community shape of tests/test_gpu_metagenome.py
(three samples, k = 21): kernel-family times from bbk_ctx_profile_get (device events) and wall times around calls that
end in a synchronise, next to the wall time of the CPU restatement (tests/kmerprofile_restated.py: Python, NOT the
reference binary) on the same input.  Prints one JSON line.

    python tools/kmerprofile_perf.py [--reads 6000] [--repeats 5] [--no-cpu]
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

JOIN = ("kp_filter", "kp_scatter", "kp_keep", "kp_compact")
ABUND = ("ab_collect", "ab_reduce")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=6000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    k, n_samples = 21, 3
    ctx = B.Context(0)
    samples = [ctx.reads_synth_meta(a.reads, read_len=150, n_genomes=20, min_len=2000, max_len=30000, sigma=2.0,
                                    sub_rate=0.005, seed=44) for _ in range(n_samples)]
    lists = [r.to_list() for r in samples]
    # the samples share the community (one seed); they differ by which third of the reads they hold twice
    third = a.reads // 3
    lists = [l + l[s * third:(s + 1) * third] for s, l in enumerate(lists)]
    samples = [ctx.reads_from_ascii(l) for l in lists]
    sets = [ctx.count(r, k, B.CANONICAL | B.WITH_COUNTS) for r in samples]
    pooled = ctx.reads_from_ascii([r for l in lists for r in l])
    unitigs = ctx.unitigs(ctx.extindex(pooled, k))
    contigs = unitigs.to_reads()

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

    prof, join_t = timed(lambda: ctx.kmerprofile(k, sets, 1), JOIN)
    res, ab_t = timed(lambda: prof.abundance(contigs), ABUND)
    out = {"k": k, "samples": n_samples, "reads_per_sample": len(lists[0]),
           "distinct_per_sample": [len(s) for s in sets], "kept_kmers": len(prof), "contigs": len(contigs),
           "contig_positions": int(res[1].sum()), "found": int(res[0].sum()), "join": join_t, "abundance": ab_t}
    if not a.no_cpu:
        from tests import kmerprofile_restated as R
        exported = [s.export(with_counts=True) for s in sets]
        t0 = time.perf_counter()
        rk, rr = R.join([R.filter_sample(keys, cnt) for keys, cnt in exported], 1, 5)
        out["cpu_python_restatement_join_s"] = time.perf_counter() - t0
        table = {R.decode(key, k): row for key, row in zip(rk, rr)}
        seqs = unitigs.sequences()
        t0 = time.perf_counter()
        exp = [R.abundance_ints(s, k, table, n_samples) for s in seqs]
        out["cpu_python_restatement_abundance_s"] = time.perf_counter() - t0
        out["equal_to_restatement"] = bool(len(rk) == len(prof) and [e[0] for e in exp] == res[0].tolist()
                                           and [e[2] for e in exp] == res[2].tolist())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
