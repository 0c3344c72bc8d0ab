"""Times the fill of BayesHammer's per-k-mer statistics (KmerStats.push) over the both-strand 21-mers of synthetic reads
with 0.5 % substitutions and host-drawn qualities in [2, 41]: the time of k_ks_accum and k_ks_finish from
bbk_ctx_profile_get (device events), k-mer positions per second, the wall time of the push, and as the yardstick the
wall time of bbk_reads_median_filter on the same reads over their canonical set with counts -- the existing
one-lookup-per-position kernel of the same shape (one wavefront per read, lanes over positions); its call also builds
its prefix table and copies one byte per read back.  Prints one JSON line.

    python tools/kmerdata_perf.py [--reads 2000000] [--repeats 5]
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
    canon = ctx.count(reads, k, B.CANONICAL | B.WITH_COUNTS)
    positions = a.reads * (a.read_len - k + 1)

    def fill():
        ks = kset.kmer_stats()
        ctx.synchronize()
        t0 = time.perf_counter()
        ks.push(reads, quals)
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ks.finish()
        return ks, wall

    ks, _ = fill()  # warm-up: code objects, arena growth
    ctx.profile(True)
    accum, finish, walls = [], [], []
    for _ in range(a.repeats):
        ks.free()
        ctx.profile_reset()
        ks, wall = fill()
        walls.append(wall)
        accum.append(ctx.profile_get("k_ks_accum")["ms"])
        finish.append(ctx.profile_get("k_ks_finish")["ms"])
    ctx.profile(False)
    cnt, tq, _ = ks.export()
    ctx.median_filter(reads, canon, 2)
    filt = []
    for _ in range(a.repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.median_filter(reads, canon, 2)
        filt.append((time.perf_counter() - t0) * 1e3)
    acc_ms = float(np.median(accum))
    out = {"k": k, "reads": a.reads, "read_len": a.read_len, "n": len(kset), "n_canonical": len(canon),
           "positions": positions, "occurrences_merged": int(cnt.sum(dtype=np.uint64)),
           "max_count": int(cnt.max()), "total_qual_zero": int((tq == 0).sum()),
           "k_ks_accum_ms_median": acc_ms, "k_ks_accum_ms_min": min(accum), "k_ks_finish_ms_median": float(np.median(finish)),
           "push_wall_ms_median": float(np.median(walls)), "positions_per_s": positions / (acc_ms * 1e-3),
           "median_filter_wall_ms_median": float(np.median(filt)), "median_filter_wall_ms_min": min(filt),
           "accum_over_median_filter": acc_ms / float(np.median(filt))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
