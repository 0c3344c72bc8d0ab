"""Times the expansion of the solid k-mers (Expander, csrc/expand.hip) over the both-strand 21-mers of synthetic reads
with 0.5 % substitutions: good at first are the k-mers that occur at least twice, and the rounds run to the closure.
Per round the time of k_ex_round and of k_ex_changed from bbk_ctx_profile_get (device events), the counts, k-mer
positions per second of the first round, and as the yardstick bbk_reads_median_filter on the same reads over their
canonical set with counts -- the one-lookup-per-position kernel of the same shape (one wavefront per read, lanes over
positions), which also takes the reverse complement of every k-mer and gathers a count where the expander gathers a
byte: the time of its kernel (device events) and the wall time of its call, which also builds its prefix table and copies
one byte per read back.  Prints one JSON line.

    python tools/expander_perf.py [--reads 2000000] [--repeats 5]
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
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-rounds", type=int, default=100)
    a = ap.parse_args()
    k = 21
    ctx = B.Context(0)
    reads = ctx.reads_synth(a.reads, read_len=a.read_len, sub_rate=0.005)
    kset = ctx.count(reads, k, B.BOTH_STRANDS | B.WITH_COUNTS)
    canon = ctx.count(reads, k, B.CANONICAL | B.WITH_COUNTS)
    n = len(kset)
    d_keys = torch.empty(n, dtype=torch.int64, device="cuda")
    d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    kset.export_to(d_keys, dst_counts=d_cnt)
    good = (d_cnt >= 2).to(torch.uint8).cpu().numpy()
    del d_keys, d_cnt
    positions = a.reads * (a.read_len - k + 1)

    def closure(timed):
        e = kset.expander(good)
        rounds = []
        while len(rounds) < a.max_rounds:
            ctx.profile_reset()
            e.begin_round()
            e.push(reads)
            c = e.end_round()
            rounds.append({"changed": c, "k_ex_round_ms": ctx.profile_get("k_ex_round")["ms"],
                           "k_ex_changed_ms": ctx.profile_get("k_ex_changed")["ms"]} if timed else {"changed": c})
            if c == 0:
                break
        total = e.good
        e.free()
        return rounds, total

    closure(False)  # warm-up: code objects, arena growth
    ctx.profile(True)
    runs = [closure(True) for _ in range(a.repeats)]
    assert all(r[1] == runs[0][1] and [x["changed"] for x in r[0]] == [x["changed"] for x in runs[0][0]] for r in runs)
    ctx.median_filter(reads, canon, 2)
    filt_wall, filt_kernel = [], []
    for _ in range(a.repeats):
        ctx.synchronize()
        ctx.profile_reset()
        t0 = time.perf_counter()
        ctx.median_filter(reads, canon, 2)
        filt_wall.append((time.perf_counter() - t0) * 1e3)
        filt_kernel.append(ctx.profile_get("k_median_filter")["ms"])
    ctx.profile(False)
    nr = len(runs[0][0])
    per_round = [{"changed": runs[0][0][r]["changed"],
                  "k_ex_round_ms_median": float(np.median([x[0][r]["k_ex_round_ms"] for x in runs])),
                  "k_ex_round_ms_min": min(x[0][r]["k_ex_round_ms"] for x in runs),
                  "k_ex_changed_ms_median": float(np.median([x[0][r]["k_ex_changed_ms"] for x in runs]))} for r in range(nr)]
    first = per_round[0]["k_ex_round_ms_median"]
    out = {"k": k, "reads": a.reads, "read_len": a.read_len, "n": n, "n_canonical": len(canon), "positions": positions,
           "good_before": int(good.sum()), "good_after": runs[0][1], "rounds": nr, "per_round": per_round,
           "first_round_positions_per_s": positions / (first * 1e-3),
           "median_filter_kernel_ms_median": float(np.median(filt_kernel)), "median_filter_kernel_ms_min": min(filt_kernel),
           "median_filter_wall_ms_median": float(np.median(filt_wall)),
           "first_round_over_median_filter_kernel": first / float(np.median(filt_kernel))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
