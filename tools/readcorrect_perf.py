"""Times the read corrector (Corrector, csrc/readcorrect.hip) on synthetic reads: a random genome, reads of it with
substitutions (1 % by default, a tenth of them an N, quality 10 at an error and 35 elsewhere), the both-strand k-mers of
the genome as the good set.  The same input goes through bbk_corrector_correct twice: with the searches on the device,
and with BBK_CORRECTOR_HOST=1, which sends every search through the host rule under OpenMP.  Per path the wall time of the
call (uploads, the island kernel, the searches, the copies back and the counters) and, from bbk_ctx_profile_get (device
events), the time of k_rc_island and k_rc_search.  The outputs of the two paths must be the same bytes.  Prints one JSON
line.

    python tools/readcorrect_perf.py [--reads 200000] [--read-len 150] [--repeats 5]
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
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome", type=int, default=1_000_000)
    ap.add_argument("--sub-rate", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    k = 21
    rng = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, a.genome)]
    starts = rng.integers(0, a.genome - a.read_len + 1, a.reads)
    bases = genome[(starts[:, None] + np.arange(a.read_len)[None, :])].reshape(-1).copy()
    err = rng.random(len(bases)) < a.sub_rate
    code = np.searchsorted(acgt, bases)
    bases[err] = acgt[(code[err] + rng.integers(1, 4, int(err.sum()))) % 4]
    bases[err & (rng.random(len(bases)) < 0.1)] = ord("N")
    qual = np.where(err, 10, 35).astype(np.uint8)
    off = (np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(a.read_len)).astype(np.uint64)

    ctx = B.Context(0)
    g = ctx.reads_from_ascii([genome.tobytes().decode()])
    kset = ctx.count(g, k, B.BOTH_STRANDS)
    n = len(kset)
    cor = kset.corrector(np.ones(n, dtype=np.uint8))

    def run(host):
        if host:
            os.environ["BBK_CORRECTOR_HOST"] = "1"
        else:
            os.environ.pop("BBK_CORRECTOR_HOST", None)
        cor.correct_arrays(bases, qual, off)  # warm-up: code objects, arena growth, the host copy of the set
        wall, island, search, out = [], [], [], None
        for _ in range(a.repeats):
            ctx.synchronize()
            ctx.profile_reset()
            t0 = time.perf_counter()
            out = cor.correct_arrays(bases, qual, off)
            wall.append((time.perf_counter() - t0) * 1e3)
            island.append(ctx.profile_get("k_rc_island")["ms"])
            search.append(0.0 if host else ctx.profile_get("k_rc_search")["ms"])
        return {"wall_ms_median": float(np.median(wall)), "wall_ms_min": min(wall),
                "k_rc_island_ms_median": float(np.median(island)), "k_rc_search_ms_median": float(np.median(search))}, out

    ctx.profile(True)
    before = cor.stats
    dev, out_dev = run(False)
    mid = cor.stats
    host, out_host = run(True)
    after = cor.stats
    ctx.profile(False)
    os.environ.pop("BBK_CORRECTOR_HOST", None)
    assert all(np.array_equal(x, y) for x, y in zip(out_dev[:2], out_host[:2]))
    calls = a.repeats + 1
    per_call = {key: (mid[key] - before[key]) // calls for key in B.Corrector.STATS}
    assert all((after[key] - mid[key]) // calls == per_call[key] for key in B.Corrector.STATS[:4])
    searched = int((out_dev[2] != 0).sum())
    print(json.dumps({"k": k, "reads": a.reads, "read_len": a.read_len, "genome": a.genome, "sub_rate": a.sub_rate, "n": n,
                      "reads_searched": searched, "reads_on_host_in_device_run": int((out_dev[2] == 2).sum()),
                      "host_searches_in_host_run": (after["host_searches"] - mid["host_searches"]) // calls,
                      "per_call": per_call, "limits": cor.limits(), "device": dev, "host": host,
                      "host_over_device_wall": host["wall_ms_median"] / dev["wall_ms_median"],
                      "device_reads_per_s": a.reads / (dev["wall_ms_median"] * 1e-3)}))


if __name__ == "__main__":
    main()
